"""The integer oracle of tests/test_hip_gemm_exact.py, proved on the CPU: the references of tests/gemm_helpers.py equal plain
torch (nn.functional.linear, autograd) bit for bit, in float32 too and in two summation orders (the sums are exact in any
order); every case's exactness bound holds; the restated launch rule puts every axis value on both ka_gemm templates; and the
comparison has teeth -- a reference with one of the mistakes such a kernel can make fails torch.equal on every case the
mistake applies to."""
import pytest
import torch
import torch.nn.functional as F

from gemm_helpers import (ALL_CHAIN, ALPHA, BWD_CASES, EXACT, FC_BATCH, GEMM_CASES, GEMM_GUARDED, GEMM_OFFSET, JOBS, MUTANTS,
                          REDUCE_SPLITS, SLICE_CASES, TRANSPOSE_SHAPES, TRANSPOSES, bf16_ties, bwd_data, chain_data, chain_ksplit,
                          chain_supported, gemm_data, gemm_ref, gemm_waves, job_data, slice_data, slice_rows, slice_sums,
                          transpose_max_tiles)

GEMM_IDS = [c.id for c in GEMM_CASES]


def logical(case, d):
    """(opA (M, K), opB (K, N)) of a GEMM case as plain float32 matrices."""
    a = d.A[:, :case.a_shape[1]]
    b = d.B[:, :case.b_shape[1]]
    return (a.t() if case.ta else a), (b.t() if case.tb else b)


# ------------------------------------------------------------------------------------------------ references against torch
@pytest.mark.parametrize("case", GEMM_CASES, ids=GEMM_IDS)
def test_gemm_reference_equals_torch_bit_for_bit(case):
    d = gemm_data(case)
    a, b = logical(case, d)
    assert float(a.abs().max()) <= 2 and float(b.abs().max()) <= 2 and torch.equal(a, a.bfloat16().float())
    for dt in (torch.float64, torch.float32):
        got = F.linear(a.to(dt), b.t().to(dt))
        flipped = F.linear(a.flip(1).to(dt), b.flip(0).t().to(dt))                     # the same sum, K walked backwards
        assert torch.equal(got, flipped)
        assert torch.equal(got.double(), sum(gemm_ref(case._replace(nsplit=1, bias=False, relu=False, accumulate=False), d.A, d.B, None, None)))
        if case.nsplit == 1:
            full = F.linear(a.to(dt), b.t().to(dt), None if d.bias is None else d.bias.to(dt))
            full = torch.relu(full) if case.relu else full
            full = full + d.target.to(dt) if d.target is not None else full
            assert torch.equal(full.double(), d.total)
        else:
            assert torch.equal(got.double(), d.total)
            for (kbeg, kend), slab in zip(case.ranges, d.slabs):
                assert torch.equal(slab, (a[:, kbeg:kend].to(dt) @ b[kbeg:kend].to(dt)).double())
    assert float(d.total.abs().max()) < EXACT and case.K * 4 + 4 < EXACT
    assert float((d.total != 0).double().mean()) > (0.3 if case.relu else 0.5) or case.K < 8, "an output of zeros would hide a dropped product"


@pytest.mark.parametrize("index", range(len(JOBS)))
def test_job_reference_equals_autograd_bit_for_bit(index):
    job, d = JOBS[index], job_data(index)
    for dt in (torch.float64, torch.float32):
        W = torch.zeros(job.N, job.K, dtype=dt, requires_grad=True)
        b = torch.zeros(job.N, dtype=dt, requires_grad=True)
        F.linear(d.x[:, :job.K].to(dt), W, b).backward(d.dy.to(dt))
        assert torch.equal(W.grad.double(), d.dW)
        assert d.db is None or torch.equal(b.grad.double(), d.db)
        assert torch.equal(W.grad, d.dy.flip(0).to(dt).t() @ d.x[:, :job.K].flip(0).to(dt)), "the same sum, rows walked backwards"
    assert job.M * 4 < EXACT and bool(torch.isnan(d.x[:, job.K:]).all())


@pytest.mark.parametrize("case", ALL_CHAIN, ids=[c.id for c in ALL_CHAIN])
def test_chain_reference_equals_two_linears_bit_for_bit(case):
    d = chain_data(case)
    for dt in (torch.float64, torch.float32):
        x = d.x[:, :case.K1].to(dt)
        xp = d.scale.to(dt) * (x * ALPHA) + d.shift.to(dt) if case.affine else x
        hidden = torch.relu(F.linear(xp, d.W1.to(dt), None if d.b1 is None else d.b1.to(dt)))
        y = F.linear(hidden, d.W2.to(dt), None if d.b2 is None else d.b2.to(dt))
        assert torch.equal(xp.double(), d.xp) and torch.equal(hidden.double(), d.hidden) and torch.equal(y.double(), d.y), dt
        hidden2 = torch.relu(F.linear(xp.flip(1), d.W1.flip(1).to(dt), None if d.b1 is None else d.b1.to(dt)))
        assert torch.equal(hidden2, hidden) and torch.equal(F.linear(hidden.flip(1), d.W2.flip(1).to(dt)), F.linear(hidden, d.W2.to(dt)))
    # the bound: multiples of 0.5 below 2^23 in magnitude are exact in fp32
    assert torch.equal(d.xp * 2, (d.xp * 2).round()) and 2 * float(d.y.abs().max()) < EXACT and 2 * float(d.hidden.abs().max()) < EXACT
    wmax = float(max(d.W1.abs().max(), d.W2.abs().max()))
    assert 2 * (case.H * (case.K1 * float(d.xp.abs().max()) * wmax + 2) * wmax + 2) < EXACT
    assert float((d.hidden > 0).double().mean()) > 0.2 and float((d.hidden == 0).double().mean()) > 0.2, "both sides of the ReLU"


@pytest.mark.parametrize("case", BWD_CASES, ids=[c.id for c in BWD_CASES])
def test_chain_backward_reference_equals_autograd_bit_for_bit(case):
    d = bwd_data(case)
    for dt in (torch.float64, torch.float32):
        x = torch.zeros(case.M, case.K1, dtype=dt, requires_grad=True)
        h = F.linear(x, d.W1.to(dt)) * (d.hidden > 0)
        h.retain_grad()
        F.linear(h, d.W2.to(dt)).backward(d.dy.to(dt))
        assert torch.equal(x.grad.double(), d.dx)
        assert torch.equal(((d.dy.to(dt) @ d.W2.to(dt)) * (d.hidden > 0)).double(), d.dh)
        assert torch.equal(((d.dy.flip(1).to(dt) @ d.W2.flip(0).to(dt)) * (d.hidden > 0)).double(), d.dh)
        assert torch.equal((d.dh.flip(1).to(dt) @ d.W1.flip(0).to(dt)).double(), d.dx)
    assert case.H * case.N2 * 4 * 2 < EXACT and chain_supported(case.N2, case.N2, case.H, case.K1)


@pytest.mark.parametrize("M,nsplit,N", SLICE_CASES)
def test_slice_sums_equal_torch_bit_for_bit(M, nsplit, N):
    A, Bm, mean, invstd = slice_data(M, nsplit, N)
    for t in (A, A * Bm, A * A, A * ((Bm - mean) * invstd)):
        parts = slice_sums(t, M, nsplit)
        assert torch.equal(parts.sum(0), t.double().sum(0)) and torch.equal(parts.float().sum(0), t.sum(0))
        assert torch.equal(parts.float().sum(0), t.flip(0).sum(0))
    assert torch.equal((A * ((Bm - mean) * invstd)).double(), A.double() * ((Bm.double() - mean.double()) * invstd.double())), "exact in fp32"


# ------------------------------------------------------------------------------------------------ the axes
def test_both_gemm_templates_meet_every_axis_value():
    """The restated ka_gemm_waves rule (no library here) classifies the tables as they claim, and each template has every
    (transA, transB) with every M, N, K, split, dtype, stride and epilogue value of the GPU test's docstring."""
    for c in GEMM_CASES + GEMM_GUARDED:
        assert gemm_waves(c.M, c.N, c.nsplit) == c.waves, c.id
    for waves in (4, 16):
        for ta, tb in TRANSPOSES:
            cs = [c for c in GEMM_CASES if (c.waves, c.ta, c.tb) == (waves, ta, tb)]
            assert {1, 15, 16, 17, 49, 63} <= {c.M % 64 for c in cs} and any(c.M < 16 for c in cs)
            assert {1, 3, 16, 17, 139} <= {c.N for c in cs} and any(c.N % 64 == 0 for c in cs)
            assert {1, 3, 4, 5, 31} <= {c.K % 32 for c in cs} and any(c.K < 32 for c in cs)
            assert {1, 2, 3, 9} <= {c.nsplit for c in cs}
            assert any(c.ranges[-1][0] == c.ranges[-1][1] for c in cs if c.K == 33 and c.nsplit == 3), "an empty last range"
            assert any(0 < c.ranges[-1][1] - c.ranges[-1][0] < c.ranges[0][1] for c in cs if c.nsplit > 1), "a short last range"
            assert any(0 < e - b < 32 for c in cs if c.nsplit > 1 for b, e in c.ranges)
            # a vector-aligned operand that must finish its rows on element loads: ld % 4 == 0 < row % 4 on both operands
            r4 = [c for c in cs if c.round4]
            assert r4 and all(c.lda % 4 == 0 and c.ldb % 4 == 0 and c.lda > c.a_shape[1] % 4 > 0 and c.b_shape[1] % 4 for c in r4)
            assert {(c.a_bf16, c.b_bf16) for c in r4} == {(False, False), (True, True)} and set(r4) <= set(GEMM_OFFSET)
            assert any(c.a_bf16 and not c.b_bf16 for c in cs) and any(c.b_bf16 and not c.a_bf16 for c in cs) and any(c.c_bf16 for c in cs)
            assert tb or any(c.N == 139 and c.ldb == 139 for c in cs), "ldb = 139 with transB = 0"
            assert any(c.ldc > c.N for c in cs)
            for combo in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                assert any((c.bias, c.relu, c.accumulate) == combo for c in cs), combo
            assert sum((g.waves, g.ta, g.tb) == (waves, ta, tb) for g in GEMM_GUARDED) == 1
    for c in GEMM_CASES:
        if c.c_bf16:
            assert bf16_ties(gemm_data(c).total) >= 1, c.id


def test_job_chain_and_slice_tables_meet_their_axes():
    assert len(JOBS) >= 12 and JOBS[0].wgs == 1 and JOBS[-1].wgs == 1 and sum(j.wgs == 1 for j in JOBS) >= 6
    assert {j.M for j in JOBS} == {1, 31, 32, 33, 97, 300} and {j.N for j in JOBS} == {3, 64, 65}
    for bias in (True, False):
        ks = {j.K for j in JOBS if j.bias == bias}
        assert {64, 128} <= ks and any(k % 64 == 63 for k in ks) and {1, 2, 3} <= {k % 4 for k in ks}, bias
    assert any(j.ldx % 4 and j.ldx > j.K for j in JOBS) and any(j.ldx % 4 == 0 and j.ldx > j.K for j in JOBS)
    assert any(j.x_bf16 and j.x_off for j in JOBS) and any(not j.x_bf16 and j.x_off for j in JOBS)
    assert all(j.wgs == 2 for j in JOBS if j.bias and j.K == 64 and j.N <= 64), "the ones column opens a tile of its own"

    cs = ALL_CHAIN
    assert {c.H for c in cs} == {16, 32, 64, 128, 256, 512} and {c.M for c in cs} == {1, 15, 16, 17, 37}
    assert {c.N2 for c in cs} == {1, 3, 16, 17, 129, 139}
    for H, smallest in ((16, 128), (32, 64), (64, 32), (128, 16)):
        assert min(c.K1 for c in cs if c.H == H) == smallest and not chain_supported(smallest - 16, smallest, H, 1)
    for ksplit_gt1 in (True, False):
        lens = {c.klen for c in cs if (chain_ksplit(c.H) > 1) == ksplit_gt1}
        assert FC_BATCH in lens and min(lens) < FC_BATCH < max(lens), lens
    assert any(c.ldx > c.K1 for c in cs) and any(c.H > FC_BATCH for c in cs)
    for name in ("b1", "b2", "affine", "hidden_out"):
        assert {getattr(c, name) for c in cs} == {True, False}, name
    assert {c.x_out for c in cs if c.affine} == {True, False}

    assert {chain_ksplit(c.H) for c in BWD_CASES} == {8, 4, 2, 1} and any(c.K1 % 16 for c in BWD_CASES)
    assert all(c.K1 == 3 * c.N2 for c in BWD_CASES[:-1]) and {c.M for c in BWD_CASES} == {1, 15, 16, 17, 37}
    for c in BWD_CASES[:4]:                      # one per ksplit class
        ksplit = chain_ksplit(c.H)
        assert not chain_supported(c.N2 - 16 * ksplit, c.N2 - 16 * ksplit, c.H, c.K1), "the smallest C of its class"

    assert {slice_rows(M, ns)[0] for M, ns, _ in SLICE_CASES} == {1, 3, 4, 5, 28, 29, 32, 33, 36, 37}
    assert {N for _, _, N in SLICE_CASES} == {1, 63, 64, 65, 139} and any(ns > M for M, ns, _ in SLICE_CASES)
    assert any(b == e for M, ns, _ in SLICE_CASES for b, e in slice_rows(M, ns)[1]), "an empty slice"
    assert transpose_max_tiles(TRANSPOSE_SHAPES) == 8 * 24 and REDUCE_SPLITS == (1, 7, 8, 9, 17)


# ------------------------------------------------------------------------------------------------ mutants of the references
@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_of_the_reference_fails_on_every_case(name):
    for passes, cases in MUTANTS[name]:
        assert len(cases) >= 1, "a mutant nothing applies to proves nothing"
        for case in cases:
            assert not passes(case), f"{name} passes on {getattr(case, 'id', case)}"


def test_mutants_meet_both_templates():
    for name in ("last_k_dropped", "ld_ignored", "trans_a_ignored", "empty_split_unwritten", "bf16_truncated"):
        assert {c.waves for c in MUTANTS[name][0][1]} == {4, 16}, name
    assert len(MUTANTS["transpose_stride_swapped"][0][1]) == 4 and len(MUTANTS["ones_column_off_by_one"][0][1]) >= 6
