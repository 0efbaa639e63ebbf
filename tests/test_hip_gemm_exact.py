"""The kernels of csrc/gemm.hip held to an exact integer oracle (tests/gemm_helpers.py): with operands in -2..2 every product
and every fp32 partial sum is exact whatever the summation order, so each output must equal the fp64 reference to the bit --
ka_gemm on BOTH templates (every case asserts ka_gemm_waves), all four transposes, row and column tails, ragged K, split-K
with short and empty ranges, bf16 operands and outputs (ties rounded to even), strides wider than the rows, pointers off their
alignment, bias / ReLU / accumulate; the grouped weight gradient with its ones column at every place of a tile; the FC chain
forward (every ksplit class, K ranges under, at and over one trip, affine input, optional outputs) and backward (the hmask
branch, weights transposed by ka_transpose_multi in the same test); the column-sum, row and slab kernels at their loop edges
and past their grid caps.  Outputs are NaN-prefilled; a single misplaced element fails.  One case per MFMA kernel on Gaussian
data bounds the accumulation error, about which exactness says nothing.  tests/test_gemm_exact_cpu.py proves the oracle."""
import pytest
import torch

from keisei_amd import _lib
from keisei_amd._lib import KeiseiHipError
from test_hip_conv_bounds import PATTERN, bits, check_guarded, guarded, guards_intact
from gemm_helpers import (ALPHA, BWD_CASES, CHAIN_CASES, CHAIN_GUARDED, GEMM_CASES, GEMM_GUARDED, GEMM_OFFSET, GRID_STRIDE_COLS,
                          GRID_STRIDE_ROWS, JOBS, NAN, REDUCE_SIZES, REDUCE_SPLITS, SLICE_CASES, TRANSPOSE_SHAPES, bwd_data, chain_data,
                          chain_ksplit, gemm_data, gemm_waves, ints, job_data, slice_data, slice_sums, transpose_max_tiles)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


def st():
    return _lib.stream_ptr()


def sync():
    torch.cuda.synchronize()


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def place(t, dtype=F32, off=0):
    """t on the device in dtype, contiguous, starting `off` elements past a 16-byte aligned address."""
    flat = torch.zeros(t.numel() + off, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    flat[off:].copy_(t.flatten().to(dtype))
    return flat[off:].view(t.shape)


def dev(t):
    return None if t is None else place(t)


def assert_same(got, expected, what):
    """torch.equal of a device result with an fp64 (or bf16) reference, rounded once to the result's dtype."""
    got = got.cpu()
    expected = expected.float().to(got.dtype) if expected.dtype == torch.float64 else expected
    if not torch.equal(got, expected):
        diff = (got.double() - expected.double()).abs().nan_to_num(nan=float("inf")).flatten()
        i = int(diff.argmax())
        pytest.fail(f"{what}: {int((diff != 0).sum())} of {diff.numel()} entries differ, worst at flat index {i} of shape "
                    f"{tuple(got.shape)}: got {float(got.flatten()[i])}, expected {float(expected.flatten()[i])}")


# ------------------------------------------------------------------------------------------------ ka_gemm
def launch_gemm(case, A, B, C, bias):
    assert _lib.query("ka_gemm_waves", case.M, case.N, case.nsplit) == case.waves == gemm_waves(case.M, case.N, case.nsplit), \
        f"{case.id}: the library would not launch the {case.waves}-wave template"
    _lib.call("ka_gemm", A, B, C, bias, case.M, case.N, case.K, case.lda, case.ldb, case.ldc, case.ta, case.tb, int(case.a_bf16),
              int(case.b_bf16), int(case.c_bf16), int(case.relu), int(case.accumulate), case.nsplit, st())


def run_gemm(case, off=False):
    """One call on pattern-filled slabs of M x ldc: every slab equal to its reference, pad columns untouched.  Returns the
    slabs (nsplit, M, N) on the device."""
    d = gemm_data(case)
    A = place(d.A, BF16 if case.a_bf16 else F32, (2 if case.a_bf16 else 1) if off else 0)
    B = place(d.B, BF16 if case.b_bf16 else F32, (2 if case.b_bf16 else 1) if off else 0)
    cdt = BF16 if case.c_bf16 else F32
    it, v = PATTERN[cdt]
    C = torch.full((case.nsplit, case.M, case.ldc), v, dtype=it, device=DEV).view(cdt)
    if case.accumulate:
        C[0, :, :case.N] = d.target.to(DEV)
    launch_gemm(case, A, B, C, dev(d.bias))
    sync()
    for s, slab in enumerate(d.slabs):
        assert_same(C[s, :, :case.N], slab, f"{case.id} slab {s} (K range {case.ranges[s]})")
    if case.ldc_pad:
        assert bool((bits(C[:, :, case.N:]) == v).all()), f"{case.id}: pad columns of C written"
    return C[:, :, :case.N]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c.id for c in GEMM_CASES])
def test_gemm_exact(case):
    """Every row of GEMM_ROWS_16 / GEMM_ROWS_4 with all four (transA, transB): the slabs to the bit (an empty K range writes
    zeros), then ka_reduce_slabs over them, overwriting NaN and accumulating onto an integer pattern."""
    slabs = run_gemm(case)
    if case.nsplit > 1:
        d = gemm_data(case)
        n = case.M * case.N
        slabs = slabs.contiguous()
        out = nans(case.M, case.N)
        _lib.call("ka_reduce_slabs", slabs, out, case.nsplit, n, 0, st())
        assert_same(out, d.total, f"{case.id} reduced")
        pattern = ints(torch.Generator().manual_seed(n), case.M, case.N, lo=-3, hi=3)
        out = place(pattern)
        _lib.call("ka_reduce_slabs", slabs, out, case.nsplit, n, 1, st())
        assert_same(out, d.total + pattern.double(), f"{case.id} reduced onto a pattern")


@pytest.mark.parametrize("case", GEMM_OFFSET, ids=[c.id for c in GEMM_OFFSET])
def test_gemm_pointer_off_alignment_gives_the_same_bits(case):
    """Rows of a multiple of four elements from an aligned pointer (vector loads, finished on element loads: the rows' own
    length is no multiple of four) and from a pointer one fp32 / two bf16 elements further (element loads only)."""
    aligned, shifted = run_gemm(case), run_gemm(case, off=True)
    assert torch.equal(aligned, shifted)


@pytest.mark.parametrize("case", GEMM_GUARDED, ids=[c.id for c in GEMM_GUARDED])
def test_gemm_between_guard_rows(case):
    """A, B, bias and C between guard rows: the same bits with zero and NaN input guards, output guards intact."""
    d = gemm_data(case)
    m = check_guarded(lambda t: launch_gemm(case, t["A"], t["B"], t["C"], t["bias"]),
                      {"A": d.A, "B": d.B, "bias": d.bias}, {"C": ((case.M, case.N), F32)})
    assert_same(m["C"], d.total, f"guarded {case.id}")


# ------------------------------------------------------------------------------------------------ grouped weight gradient
def run_jobs(order):
    """One ka_gemm_grouped_wgrad launch over the jobs in the given order, dW / db NaN-patterned between guard rows:
    index -> (dW, db) on the CPU."""
    rows, keep, wg = [], [], 0
    for i in order:
        job, d = JOBS[i], job_data(i)
        dy, x = place(d.dy), place(d.x, BF16 if job.x_bf16 else F32, job.x_off)
        fW, dW = guarded((job.N, job.K), F32, "pattern")
        fb, db = guarded((job.N,), F32, "pattern") if job.bias else (None, None)
        keep.append((i, dy, x, fW, dW, fb, db))
        rows.append([dy.data_ptr(), x.data_ptr(), dW.data_ptr(), db.data_ptr() if job.bias else 0, job.M, job.N, job.K, job.ldx,
                     int(job.x_bf16), wg])
        wg += job.wgs
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    sync()
    _lib.call("ka_gemm_grouped_wgrad", table, len(rows), wg, st())
    sync()
    out = {}
    for i, _, _, fW, dW, fb, db in keep:
        assert guards_intact(fW) and (fb is None or guards_intact(fb)), f"job {i} {JOBS[i]}: guard rows overwritten"
        assert_same(dW, job_data(i).dW, f"job {i} {JOBS[i]} dW")
        if db is not None:
            assert_same(db, job_data(i).db, f"job {i} {JOBS[i]} db")
        out[i] = (dW.cpu(), None if db is None else db.cpu())
    return out


def test_grouped_weight_gradient_exact():
    """The fifteen jobs of JOBS in one launch, then in another order (reversed, rotated by four): every dW and db to the bit
    both times."""
    n = len(JOBS)
    first = run_jobs(range(n))
    second = run_jobs([(n - 1 - i + 4) % n for i in range(n)])
    for i in range(n):
        assert torch.equal(first[i][0], second[i][0]) and (first[i][1] is None or torch.equal(first[i][1], second[i][1]))


# ------------------------------------------------------------------------------------------------ FC chain, forward
def launch_chain(case, d, x, xo, hid, y, scale=None, shift=None):
    assert _lib.query("ka_fc_chain_supported", case.K1, case.ldx, case.H, case.N2) == 1
    _lib.call("ka_fc_chain", x, scale, shift, ALPHA if case.affine else 1.0, d["W1"], d["b1"], d["W2"], d["b2"], xo, hid, y,
              case.M, case.K1, case.ldx, case.H, case.N2, st())


def chain_operands(case):
    d = chain_data(case)
    return {n: dev(getattr(d, n)) for n in ("scale", "shift", "W1", "b1", "W2", "b2")}


@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c.id for c in CHAIN_CASES])
def test_fc_chain_forward_exact(case):
    """x', hidden and y of every CHAIN_CASES row to the bit (half-integers under the affine input: alpha = 0.5)."""
    d, o = chain_data(case), chain_operands(case)
    y = nans(case.M, case.N2)
    hid = nans(case.M, case.H) if case.hidden_out else None
    xo = nans(case.M, case.K1) if case.x_out else None
    launch_chain(case, o, place(d.x), xo, hid, y, o["scale"], o["shift"])
    sync()
    if xo is not None:
        assert_same(xo, d.xp, f"{case.id} x_out")
    if hid is not None:
        assert_same(hid, d.hidden, f"{case.id} hidden_out (ksplit {chain_ksplit(case.H)})")
    assert_same(y, d.y, f"{case.id} y")


def test_fc_chain_forward_between_guard_rows():
    case = CHAIN_GUARDED
    d, o = chain_data(case), chain_operands(case)
    m = check_guarded(lambda t: launch_chain(case, o, t["x"], t["xo"], t["hid"], t["y"], o["scale"], o["shift"]), {"x": d.x},
                      {"xo": ((case.M, case.K1), F32), "hid": ((case.M, case.H), F32), "y": ((case.M, case.N2), F32)})
    assert_same(m["xo"], d.xp, "guarded x_out")
    assert_same(m["hid"], d.hidden, "guarded hidden_out")
    assert_same(m["y"], d.y, "guarded y")


@pytest.mark.parametrize("which", ["in_scale", "in_shift", "x_out"])
def test_fc_chain_refuses_vector_operands_off_their_alignment(which):
    """in_scale, in_shift and x_out are read / written as 16-byte vectors like x and the weights: a view one float past an
    aligned address is refused before any launch (the outputs keep their NaN)."""
    case = CHAIN_GUARDED
    d, o = chain_data(case), chain_operands(case)
    y, xo = nans(case.M, case.N2), nans(case.M * case.K1 + 1)
    args = {"in_scale": o["scale"], "in_shift": o["shift"], "x_out": xo[:-1]}
    args[which] = {"in_scale": place(d.scale, off=1), "in_shift": place(d.shift, off=1), "x_out": xo[1:]}[which]
    assert args[which].data_ptr() % 16 == 4
    with pytest.raises(KeiseiHipError, match="16-byte aligned"):
        launch_chain(case, o, place(d.x), args["x_out"], None, y, args["in_scale"], args["in_shift"])
    sync()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(xo).all())


# ------------------------------------------------------------------------------------------------ transposes, FC chain backward
def transpose_multi(srcs, max_tiles):
    """dst_i = src_i^T in one launch, every dst between guard rows: the dsts."""
    fulls = [guarded((s.shape[1], s.shape[0]), F32, "pattern") for s in srcs]
    table = torch.tensor([[s.data_ptr(), mid.data_ptr(), s.shape[0], s.shape[1]] for s, (_, mid) in zip(srcs, fulls)], dtype=torch.int64).to(DEV)
    sync()
    _lib.call("ka_transpose_multi", table, len(srcs), max_tiles, st())
    sync()
    for s, (full, mid) in zip(srcs, fulls):
        assert guards_intact(full), f"transpose of {tuple(s.shape)}: guard rows overwritten"
        assert torch.equal(mid, s.t()), f"transpose of {tuple(s.shape)} with max_tiles {max_tiles}"
    return [mid for _, mid in fulls]


def test_transpose_multi():
    """(1, 1) .. (256, 768) in one table: with max_tiles as _fc_transposed computes it (192: the 64-workgroup cap makes the
    large matrix go round the grid-stride loop three times while the small ones leave workgroups idle) and with 3."""
    g = torch.Generator().manual_seed(3)
    srcs = [torch.randn(r, c, generator=g).to(DEV) for r, c in TRANSPOSE_SHAPES]
    transpose_multi(srcs, transpose_max_tiles(TRANSPOSE_SHAPES))
    transpose_multi(srcs, 3)


@pytest.mark.parametrize("case", BWD_CASES, ids=[c.id for c in BWD_CASES])
def test_fc_chain_backward_exact(case):
    """dhidden = (dy W2) * [hidden > 0] and dx = dhidden W1 to the bit, the saved hidden holding positives, +0.0 and -0.0;
    W2^T and W1^T come from ka_transpose_multi as in _fc_transposed."""
    d = bwd_data(case)
    W2, W1 = place(d.W2), place(d.W1)
    w2t, w1t = transpose_multi([W2, W1], transpose_max_tiles([tuple(W2.shape), tuple(W1.shape)]))
    dh, dx = nans(case.M, case.H), nans(case.M, case.K1)
    _lib.call("ka_fc_chain_bwd", place(d.dy), place(d.hidden), w2t, w1t, dh, dx, case.M, case.N2, case.H, case.K1, st())
    sync()
    assert_same(dh, d.dh, f"{case.id} dhidden (ksplit {chain_ksplit(case.H)})")
    assert_same(dx, d.dx, f"{case.id} dx")


# ------------------------------------------------------------------------------------------------ column sums over row slices
@pytest.mark.parametrize("M,nsplit,N", SLICE_CASES)
def test_slice_sums_exact(M, nsplit, N):
    """ka_colsum (with and without Bm / part2), ka_rows_sq_sums and ka_rows_bn_sums over NaN: every slice's sums to the bit,
    empty slices exact zeros."""
    A, Bm, mean, invstd = slice_data(M, nsplit, N)
    a, b = place(A), place(Bm)
    what = f"M {M} in {nsplit} slices, N {N}"
    p1, p2 = nans(nsplit, N), nans(nsplit, N)
    _lib.call("ka_colsum", a, b, p1, p2, M, N, nsplit, st())
    assert_same(p1, slice_sums(A, M, nsplit), "colsum, " + what)
    assert_same(p2, slice_sums(A.double() * Bm.double(), M, nsplit), "colsum part2, " + what)
    p1 = nans(nsplit, N)
    _lib.call("ka_colsum", a, None, p1, None, M, N, nsplit, st())
    assert_same(p1, slice_sums(A, M, nsplit), "colsum alone, " + what)
    p1, p2 = nans(nsplit, N), nans(nsplit, N)
    _lib.call("ka_rows_sq_sums", a, p1, p2, M, N, nsplit, st())
    assert_same(p1, slice_sums(A, M, nsplit), "rows_sq_sums, " + what)
    assert_same(p2, slice_sums(A.double() ** 2, M, nsplit), "rows_sq_sums part2, " + what)
    p1, p2 = nans(nsplit, N), nans(nsplit, N)
    _lib.call("ka_rows_bn_sums", a, b, place(mean), place(invstd), p1, p2, M, N, nsplit, st())
    assert_same(p1, slice_sums(A, M, nsplit), "rows_bn_sums, " + what)
    assert_same(p2, slice_sums(A.double() * ((Bm.double() - mean.double()) * invstd.double()), M, nsplit), "rows_bn_sums part2, " + what)


# ------------------------------------------------------------------------------------------------ row and slab kernels
ROW_SHAPES = ((37, GRID_STRIDE_COLS), (GRID_STRIDE_ROWS, GRID_STRIDE_COLS))


@pytest.mark.parametrize("M,N", ROW_SHAPES, ids=["small", "grid-stride"])
def test_row_kernels_exact(M, N):
    """ka_rows_bn_bwd (mode 0: the pre-activation hits exactly 0 and a NaN, both masked; mode 1), ka_rows_affine_relu,
    ka_affine_rows (more than 7 rows) and ka_relu_mask (-0.0 and NaN in h) on integers; 8200 x 139 is past every grid cap
    (4096, 2048 and 1024 workgroups of 256), so each grid-stride loop goes round again."""
    assert M == 37 or M * N > 4096 * 256
    g = torch.Generator().manual_seed(M)
    dr, x, k = ints(g, M, N), ints(g, M, N), ints(g, 3 * N)
    scale, shift = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (N,), generator=g)], ints(g, N)
    x_nan = x.clone()
    x_nan[M // 2, N // 3] = NAN
    x_nan[M - 1, N - 1] = NAN
    pre = x_nan.double() * scale.double() + shift.double()
    assert bool((pre == 0).any()) and bool((pre > 0).any()) and bool((pre < 0).any())
    out = place(dr)
    _lib.call("ka_rows_bn_bwd", out, place(x_nan), place(scale), place(shift), M, N, 0, st())
    assert_same(out, torch.where(pre > 0, dr.double(), torch.zeros((), dtype=torch.float64)), "rows_bn_bwd mode 0")
    out = place(dr)
    _lib.call("ka_rows_bn_bwd", out, place(x), place(k), None, M, N, 1, st())
    assert_same(out, k[:N].double() * dr.double() + k[N:2 * N].double() + k[2 * N:].double() * x.double(), "rows_bn_bwd mode 1")
    out = nans(M, N)
    _lib.call("ka_rows_affine_relu", place(x), place(scale), place(shift), out, M, N, st())
    assert_same(out, torch.relu(x.double() * scale.double() + shift.double()), "rows_affine_relu")
    out = nans(M, N)
    _lib.call("ka_affine_rows", place(x), place(scale), place(shift), 0.5, out, M, N, st())
    assert_same(out, scale.double() * (x.double() * 0.5) + shift.double(), "affine_rows")
    h = torch.where((x == 0) & (torch.randint(0, 2, (M, N), generator=g) == 1), torch.tensor(-0.0), x)
    h[x_nan.isnan()] = NAN
    assert bool(torch.signbit(h[h == 0]).any()) and not bool(torch.signbit(h[h == 0]).all()) and bool(h.isnan().any())
    out = place(dr)
    _lib.call("ka_relu_mask", out, place(h), M * N, st())
    assert_same(out, torch.where(h > 0, dr.double(), torch.zeros((), dtype=torch.float64)), "relu_mask")


REDUCE_CASES = [(ns, n) for ns in REDUCE_SPLITS for n in REDUCE_SIZES] + [(9, 2048 * 256 + 77)]


@pytest.mark.parametrize("nsplit,n", REDUCE_CASES)
def test_reduce_slabs_exact(nsplit, n):
    """ka_reduce_slabs, overwriting NaN and accumulating, and ka_reduce_slabs2 against two ka_reduce_slabs calls; 2048 * 256 + 77
    elements are past the grid cap."""
    g = torch.Generator().manual_seed(nsplit * 1000 + n)
    sa, sb, pattern = ints(g, nsplit, n), ints(g, nsplit, n + 2), ints(g, 1, n, lo=-3, hi=3)
    da, db = place(sa), place(sb)
    out = nans(n)
    _lib.call("ka_reduce_slabs", da, out, nsplit, n, 0, st())
    assert_same(out, sa.double().sum(0), "reduce_slabs")
    acc = place(pattern[0])
    _lib.call("ka_reduce_slabs", da, acc, nsplit, n, 1, st())
    assert_same(acc, sa.double().sum(0) + pattern[0].double(), "reduce_slabs accumulating")
    outb, pa, pb = nans(n + 2), nans(n), nans(n + 2)
    _lib.call("ka_reduce_slabs", db, outb, nsplit, n + 2, 0, st())
    _lib.call("ka_reduce_slabs2", da, pa, n, db, pb, n + 2, nsplit, st())
    assert_same(pb, sb.double().sum(0), "reduce_slabs2 second set")
    assert torch.equal(pa, out) and torch.equal(pb, outb)


# ------------------------------------------------------------------------------------------------ rounding, Gaussian data
SEQ_FACTOR = 4      # a matrix pipe that truncates where the CPU rounds (twice the unit error) x a twofold spread between orders
                    # (the factor and its rationale are those of tests/test_hip_wgrad_exact.py)
FLOOR = 2.0 ** -22  # of the largest output entry: a quarter of its last place


def seq_matmul(a, b):
    """a (M, K) @ b (K, N) in float32, one k at a time: the plainest fp32 evaluation of the same sums."""
    acc = torch.zeros(a.shape[0], b.shape[1])
    for k in range(a.shape[1]):
        acc += torch.outer(a[:, k], b[k])
    return acc


def check_seq(name, got, ref, seq):
    """max |got - ref| <= max(SEQ_FACTOR * e_seq, FLOOR * max |ref|), e_seq = max |seq - ref|; prints the ratio."""
    err, e_seq, scale = float((got.cpu().double() - ref).abs().max()), float((seq.double() - ref).abs().max()), float(ref.abs().max())
    print(f"\n{name}: max err {err:.3e} = {err / e_seq:.2f} e_seq (e_seq = {e_seq:.3e} = {e_seq / scale:.3e} max|ref|)")
    assert err <= max(SEQ_FACTOR * e_seq, FLOOR * scale), f"{name}: max err {err:.3e} > {SEQ_FACTOR} x e_seq = {SEQ_FACTOR * e_seq:.3e}"


@pytest.mark.parametrize("waves,M,N", [(16, 37, 50), (4, 1025, 512)])
def test_gemm_accumulation_error_on_gaussian_data(waves, M, N):
    """fp32 N(0, 1) operands, K = 768, C = A B^T: within 4 x e_seq of the fp64 reference on both templates.

    Measured on an MI355X, max |C - ref64| / e_seq: 16 waves, 37 x 50: 1.00; 4 waves, 1025 x 512: 0.96."""
    K = 768
    g = torch.Generator().manual_seed(M + N)
    a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    assert _lib.query("ka_gemm_waves", M, N, 1) == waves
    C = nans(M, N)
    _lib.call("ka_gemm", a.to(DEV), b.to(DEV), C, None, M, N, K, K, K, N, 0, 1, 0, 0, 0, 0, 0, 1, st())
    check_seq(f"ka_gemm, {waves} waves", C, a.double() @ b.double().t(), seq_matmul(a, b.t()))


def test_grouped_weight_gradient_accumulation_error_on_gaussian_data():
    """One job, 768 rows of N(0, 1): dW (64 x 100) and db within 4 x e_seq of fp64.

    Measured on an MI355X, max err / e_seq: dW 1.02, db 1.00."""
    M, N, K = 768, 64, 100
    g = torch.Generator().manual_seed(M)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    dyd, xd, dW, db = dy.to(DEV), x.to(DEV), nans(N, K), nans(N)
    table = torch.tensor([[dyd.data_ptr(), xd.data_ptr(), dW.data_ptr(), db.data_ptr(), M, N, K, K, 0, 0]], dtype=torch.int64).to(DEV)
    _lib.call("ka_gemm_grouped_wgrad", table, 1, 2, st())
    check_seq("grouped dW", dW, dy.double().t() @ x.double(), seq_matmul(dy.t(), x))
    check_seq("grouped db", db, dy.double().sum(0), seq_matmul(dy.t(), torch.ones(M, 1))[:, 0])


def test_fc_chain_accumulation_error_on_gaussian_data():
    """Forward chain 768 -> 128 -> 139 on 37 rows of N(0, 1), weights and biases N(0, 1): hidden and y within 4 x e_seq.

    Measured on an MI355X, max err / e_seq: hidden 0.90, y 1.00."""
    M, K1, H, N2 = 37, 768, 128, 139
    g = torch.Generator().manual_seed(K1)
    x, W1, b1, W2, b2 = (torch.randn(*s, generator=g) for s in ((M, K1), (H, K1), (H,), (N2, H), (N2,)))
    hid, y = nans(M, H), nans(M, N2)
    _lib.call("ka_fc_chain", x.to(DEV), None, None, 1.0, W1.to(DEV), b1.to(DEV), W2.to(DEV), b2.to(DEV), None, hid, y, M, K1, K1, H, N2, st())
    hid64 = torch.relu(x.double() @ W1.double().t() + b1.double())
    hid_seq = torch.relu(seq_matmul(x, W1.t()) + b1)
    check_seq("fc_chain hidden", hid, hid64, hid_seq)
    check_seq("fc_chain y", y, hid64 @ W2.double().t() + b2.double(), seq_matmul(hid_seq, W2.t()) + b2)


def test_fc_chain_backward_accumulation_error_on_gaussian_data():
    """Backward chain, dy 37 x 768 -> dhidden (128) -> dx (64), N(0, 1) everywhere, the mask from a Gaussian hidden.

    Measured on an MI355X, max err / e_seq: dhidden 1.18, dx 0.86."""
    M, N2, H, K1 = 37, 768, 128, 64
    g = torch.Generator().manual_seed(N2 + 1)
    dy, hidden, W2, W1 = (torch.randn(*s, generator=g) for s in ((M, N2), (M, H), (N2, H), (H, K1)))
    dh, dx = nans(M, H), nans(M, K1)
    _lib.call("ka_fc_chain_bwd", dy.to(DEV), hidden.to(DEV), W2.t().contiguous().to(DEV), W1.t().contiguous().to(DEV), dh, dx,
              M, N2, H, K1, st())
    dh64 = (dy.double() @ W2.double()) * (hidden > 0)
    dh_seq = seq_matmul(dy, W2) * (hidden > 0)
    check_seq("fc_chain_bwd dhidden", dh, dh64, dh_seq)
    check_seq("fc_chain_bwd dx", dx, dh64 @ W1.double(), seq_matmul(dh_seq, W1))
