"""ka_conv3x3_wgrad held to an exact integer oracle (tests/wgrad_helpers.py): with small-integer operands every product and
every fp32 partial sum is exact whatever the summation order, so dW must equal the fp64 reference to the bit on every kernel
form -- the lean bf16 kernel, the tiled bf16 kernel at both tile widths, staggered staging on and off, fp32 at both tile widths
-- and a single misplaced product fails.  The cases reach what one board per split never does: board ranges longer than one
board (the three-tile ring, k-steps that straddle two boards, the pad rows of the last step), partial tiles under such ranges,
padded input channels that hold data, and every combination of the fused input transform.  One case on Gaussian data bounds
the accumulation error, about which exactness says nothing.  tests/test_wgrad_exact_cpu.py proves the oracle on the CPU."""
import functools

import pytest
import torch

from keisei_amd import _lib
from test_hip_conv_bounds import check_guarded
from wgrad_helpers import (FORMS, GEOMETRY_CASES, RANGE_CASES, ROUTES, SWITCHES, TRANSFORM_CASES, accumulate_pattern, case_data,
                           ranges_of, ref64, seq_f32_error, split_plan)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def st():
    return _lib.stream_ptr()


def routes():
    out = torch.zeros(len(ROUTES), dtype=torch.int64)
    _lib.call("ka_conv_route_counts", out.data_ptr(), len(ROUTES))
    return out


def select(ka_env, form):
    for name in SWITCHES:
        if name in form.env:
            ka_env.set(name, form.env[name])
        else:
            ka_env.unset(name)


def launch(form, t, B, Cin, Cin_real, Cout, relu, accumulate, target_wgs):
    """One ka_conv3x3_wgrad call on the tensors of t; the form's route counter must rise by one and the other one stay."""
    before = routes()
    _lib.call("ka_conv3x3_wgrad", t["dy"], t["x"], t.get("scale"), t.get("shift"), t.get("bias"), int(relu), t["slab"], t["dw"],
              B, Cin, Cin_real, Cout, int(accumulate), target_wgs, _lib.dtype_code(form.dtype), st())
    rose = {n: int(d) for n, d in zip(ROUTES, routes() - before) if d}
    assert rose == {form.route: 1}, f"{form.name}: expected one launch on {form.route}, counters rose by {rose}"


@functools.lru_cache(maxsize=None)
def device_operands(case, dtype):
    """The case's operands on the device: dy and x in the form's dtype, the coefficients in fp32 (shared by the forms)."""
    op, _ = case_data(case)
    t = {"dy": op.dy.to(DEV, dtype), "x": op.x.to(DEV, dtype)}
    for name in ("scale", "shift", "bias"):
        if getattr(op, name) is not None:
            t[name] = getattr(op, name).to(DEV)
    return t


def check_plan(case):
    nsplit, bps, lengths = case.plan
    assert tuple(lengths) == case.lengths, f"{case.id}: the split plan {lengths} is not the one the case claims"
    assert nsplit == _lib.query("ka_wgrad_splits", case.B, case.Cin, case.Cout, case.target_wgs), \
        f"{case.id}: the library's split count differs from split_plan's {nsplit}"
    return nsplit


def explain(case, form, got, expected, slab):
    """The failure message: form, split plan, worst (n, c, tap), and the splits of the slab ([split][tap][n][c]) that differ
    from the partial gradient of their own board range."""
    op, _ = case_data(case)
    diff = (got.double() - expected.double()).abs().nan_to_num(nan=float("inf"))
    n, c, tap = (int(v) for v in torch.unravel_index(diff.argmax(), diff.shape[:2] + (9,)))
    flat = diff.reshape(*diff.shape[:2], 9)
    bad = []
    parts = slab.cpu().reshape(case.plan[0], 9, case.Cout, case.Cin)
    for s, (beg, end) in enumerate(ranges_of(case.plan)):
        bias = None if op.bias is None else op.bias[beg:end]
        part = ref64(op.x[beg:end], op.dy[beg:end], op.scale, op.shift, op.relu, bias).reshape(case.Cout, case.Cin, 9).permute(2, 0, 1)
        if not torch.equal(parts[s].double(), part):
            bad.append(s)
    return (f"{form.name} on {case.id}: plan (nsplit, boards per split, ranges) = {case.plan}; {int((flat != 0).sum())} of {flat.numel()} "
            f"entries differ, worst (n, c, tap) = ({n}, {c}, {tap}): got {float(got[n, c, tap // 3, tap % 3])}, expected "
            f"{float(expected[n, c, tap // 3, tap % 3])}; slab splits that differ from their own range's gradient: {bad}")


def run(case, form, accumulate):
    """One call on a NaN-filled slab of exactly nsplit * 9 * Cout * Cin floats and a dW of NaN (accumulating: of an integer
    pattern): dW must equal the reference (plus the pattern) bit for bit."""
    nsplit = check_plan(case)
    _, ref = case_data(case)
    expected = ref[:, :case.Cin_real].float()
    t = dict(device_operands(case, form.dtype))
    t["slab"] = torch.full((nsplit * 9 * case.Cout * case.Cin,), float("nan"), device=DEV)
    if accumulate:
        pattern = accumulate_pattern(case)
        t["dw"], expected = pattern.to(DEV), pattern + expected
    else:
        t["dw"] = torch.full((case.Cout, case.Cin_real, 3, 3), float("nan"), device=DEV)
    launch(form, t, case.B, case.Cin, case.Cin_real, case.Cout, case_data(case)[0].relu, accumulate, case.target_wgs)
    got = t["dw"].cpu()
    if not torch.equal(got, expected):
        pytest.fail(explain(case, form, got, expected, t["slab"]))
    return got


def run_guarded(case, form):
    """The same call with dy, x and the per-board bias between guard rows of zeros, then of NaN, and dW and the slab between
    pattern guards: guards intact, dW the same in both runs and equal to the reference."""
    nsplit = check_plan(case)
    op, ref = case_data(case)
    fixed = device_operands(case, form.dtype)
    inputs = {n: fixed[n] for n in ("dy", "x", "bias") if n in fixed}
    outputs = {"dw": ((case.Cout, case.Cin_real, 3, 3), torch.float32), "slab": ((nsplit * 9 * case.Cout, case.Cin), torch.float32)}
    m = check_guarded(lambda t: launch(form, {**fixed, **t}, case.B, case.Cin, case.Cin_real, case.Cout, op.relu, 0, case.target_wgs),
                      inputs, outputs, finite={"dw"})
    got, expected = m["dw"].cpu(), ref[:, :case.Cin_real].float()
    if not torch.equal(got, expected):
        pytest.fail("guarded: " + explain(case, form, got, expected, m["slab"]))


def ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", RANGE_CASES, ids=ids(RANGE_CASES))
def test_board_range_lengths(ka_env, case):
    """(a) One 64 x 64 tile, nsplit = min(target_wgs, B): ranges of 1, 2, 3, 4, 32, 33 and 35 boards, a short last split,
    padding workgroups and more than eight splits, on every form, plain input and the full transform."""
    for form in FORMS:
        select(ka_env, form)
        run(case, form, accumulate=False)


@pytest.mark.parametrize("case", GEOMETRY_CASES, ids=ids(GEOMETRY_CASES))
def test_channel_geometry(ka_env, case):
    """(b) Two ranges of four boards under partial n- and c-tiles, whole tiles (256 x 256) and padded input channels that hold
    nonzero data (dW has Cin_real channels and must not see them): every form, overwrite and accumulate, and once more between
    guard rows."""
    if case.Cin_real < case.Cin:
        op, _ = case_data(case)
        assert float(op.x[:, :, case.Cin_real:].abs().max()) > 0
    for form in FORMS:
        select(ka_env, form)
        run(case, form, accumulate=False)
        run(case, form, accumulate=True)
        run_guarded(case, form)


@pytest.mark.parametrize("case", TRANSFORM_CASES, ids=ids(TRANSFORM_CASES))
def test_transform_combinations(ka_env, case):
    """(c) Each combination of scale + shift, relu and per-board bias the ABI admits, 80 -> 144 channels, two ranges of four."""
    for form in FORMS:
        select(ka_env, form)
        run(case, form, accumulate=False)


# ------------------------------------------------------------------------------------------------ rounding, Gaussian data
SEQ_FACTOR = 4      # a matrix pipe that truncates where the CPU rounds (twice the unit error) x a twofold spread between orders


@pytest.mark.parametrize("B,C,target_wgs,lengths", [(35, 64, 1, (35,)), (40, 256, 16, (20, 20))], ids=["B35-64x64", "B40-256x256"])
def test_accumulation_error_on_gaussian_data(ka_env, B, C, target_wgs, lengths):
    """(d) Plain input, bf16-rounded N(0, 1) x and N(0, 1) / 9 dy (the fp32 forms get the same values): every form within
    4 x e_seq of the fp64 reference, e_seq = the error of a float32 accumulation of the 81 B row outer products one at a time
    (about 1.2e-6 max|dW|), and the lean and KA_WGRAD_LEAN=0 results bit-identical.

    Measured on an MI355X, max |dw - ref64| / e_seq:
      64 x 64, B = 35, one range (e_seq = 1.47e-6 max|dW|):     bf16 128-wide forms 0.65, bf16 64-wide 0.51, both fp32 forms 1.00
      256 x 256, B = 40, ranges 20 + 20 (e_seq = 1.68e-6 max|dW|): bf16 128-wide forms 0.27, bf16 64-wide 0.26, both fp32 forms 0.40
    (the four 128-wide bf16 forms agree to the digit shown: staggered staging does not change the order of the sum; the fp32
    kernel on a single range lands on e_seq itself, 3.218e-5 against 3.218e-5)."""
    nsplit, _, got_lengths = split_plan(B, C, C, target_wgs)
    assert tuple(got_lengths) == lengths and nsplit == _lib.query("ka_wgrad_splits", B, C, C, target_wgs)
    g = torch.Generator().manual_seed(B + C)
    x = torch.randn(B, 81, C, generator=g).to(torch.bfloat16)
    dy = (torch.randn(B, 81, C, generator=g) / 9).to(torch.bfloat16)
    ref = ref64(x, dy)
    e_seq, scale = seq_f32_error(x, dy, ref), float(ref.abs().max())
    print(f"\nB={B} C={C}: e_seq = {e_seq:.3e} = {e_seq / scale:.3e} max|dW|")
    results, errs = {}, {}
    for form in FORMS:
        select(ka_env, form)
        t = {"dy": dy.to(DEV, form.dtype), "x": x.to(DEV, form.dtype), "slab": torch.full((nsplit * 9 * C * C,), float("nan"), device=DEV),
             "dw": torch.full((C, C, 3, 3), float("nan"), device=DEV)}
        launch(form, t, B, C, C, C, 0, 0, target_wgs)
        results[form.name] = t["dw"].cpu()
        errs[form.name] = float((results[form.name].double() - ref).abs().max())
        print(f"  {form.name}: max err {errs[form.name]:.3e} = {errs[form.name] / e_seq:.2f} e_seq")
    assert torch.equal(results["bf16-lean"], results["bf16-tiled"]), "the lean and the tiled 128-wide kernels differ"
    assert torch.equal(results["bf16-lean-nostag"], results["bf16-tiled-nostag"])
    for name, err in errs.items():
        assert err <= SEQ_FACTOR * e_seq, f"{name}: max err {err:.3e} > {SEQ_FACTOR} x e_seq = {SEQ_FACTOR * e_seq:.3e}"
