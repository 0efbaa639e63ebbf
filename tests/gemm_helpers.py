"""Shared by tests/test_gemm_exact_cpu.py and tests/test_hip_gemm_exact.py: integer-valued operands of the kernels of
csrc/gemm.hip (ka_gemm on both templates, the grouped weight gradient, the FC chain forward and backward, the transposes, the
row and slab kernels), their fp64 references stated from the ABI, restatements of the library's launch rules, the mutants of
the references, and the case lists.

Why integers: these kernels run exact-f32 MFMAs (or plain fp32 adds) on operands widened to fp32.  With values in -2..2 every
product is exact and every partial sum is an integer (a half-integer in the affine chain) far below 2^23, so fp32 addition is
exact in ANY order: the result must equal the fp64 reference to the bit whatever the template, the split count, the load path
or the order of a reduce, and one dropped, doubled or misplaced element changes it."""
import functools
from typing import NamedTuple, Optional, Tuple

import torch

NAN = float("nan")
EXACT = 2 ** 23                                  # every |partial sum| (in units of 0.5 where half-integers occur) stays below this


def ceil_div(a, b):
    return -(-a // b)


def ints(g, *shape, lo=-2, hi=2):
    """Integers in lo..hi as float32; the last row and the last column hold no zero (a dropped edge always shows)."""
    t = torch.randint(lo, hi + 1, shape, generator=g).float()
    if t.ndim == 2:
        t[-1][t[-1] == 0] = 1.0
        t[:, -1][t[:, -1] == 0] = -1.0
    return t


def padded(t, ld):
    """(rows, cols) -> (rows, ld) with NaN in the pad columns: whatever reads past a row's end shows."""
    out = torch.full((t.shape[0], ld), NAN)
    out[:, :t.shape[1]] = t
    return out


def bf16_ties(ref):
    """How many entries of an integer-valued fp64 tensor lie exactly half way between two bf16 values."""
    return int(((ref.float().contiguous().view(torch.int32) & 0xFFFF) == 0x8000).sum())


def bf16_truncated(ref):
    f = ref.float().contiguous()
    return (f.view(torch.int32) & -65536).view(torch.float32).bfloat16()


# ------------------------------------------------------------------------------------------------ ka_gemm
def gemm_waves(M, N, nsplit):
    """ka_gemm_waves of csrc/gemm.hip restated: 16 waves per workgroup below 128 workgroups, else 4."""
    return 16 if ceil_div(N, 64) * ceil_div(M, 64) * nsplit < 128 else 4


def split_ranges(K, nsplit):
    """[(kbeg, kend)] of ka_gemm's K ranges: ceil(K / nsplit) rounded up to 32 each; trailing ranges may be short or empty."""
    ln = ceil_div(ceil_div(K, nsplit), 32) * 32
    return [(min(K, s * ln), min(K, (s + 1) * ln)) for s in range(nsplit)]


class GemmCase(NamedTuple):
    waves: int                                   # the template the case claims to reach
    M: int
    N: int
    K: int
    ta: int
    tb: int
    nsplit: int = 1
    a_bf16: bool = False
    b_bf16: bool = False
    c_bf16: bool = False
    round4: bool = False                         # both operands' rows padded to the next multiple of 4 elements (ld % 4 == 0, ld > row)
    ldc_pad: int = 0
    bias: bool = False
    relu: bool = False
    accumulate: bool = False
    big: bool = False                            # sign-coherent operands: results of about 1.4 K, so bf16 rounding has ties

    @property
    def id(self):
        flags = "".join(f"-{n}" for n in ("a_bf16", "b_bf16", "c_bf16", "round4", "bias", "relu", "accumulate", "big") if getattr(self, n))
        return f"w{self.waves}-{self.M}x{self.N}x{self.K}-t{self.ta}{self.tb}-s{self.nsplit}{flags}" + (f"-ldc+{self.ldc_pad}" if self.ldc_pad else "")

    @property
    def a_shape(self):                           # (rows, row length) of A as stored
        return (self.K, self.M) if self.ta else (self.M, self.K)

    @property
    def b_shape(self):
        return (self.N, self.K) if self.tb else (self.K, self.N)

    def _ld(self, row):
        return row + 4 - row % 4 if self.round4 else row

    @property
    def lda(self):
        return self._ld(self.a_shape[1])

    @property
    def ldb(self):
        return self._ld(self.b_shape[1])

    @property
    def ldc(self):
        return self.N + self.ldc_pad

    @property
    def ranges(self):
        return split_ranges(self.K, self.nsplit)


# Rows of the case tables: (M, N, K, nsplit, options); every row runs with all four (transA, transB).
#
# 16 waves: ceil(M/64) * ceil(N/64) * nsplit < 128 -- the small shapes of test_gemm_variants and their neighbours.
#   M % 64: 37, 1 (65), 15 (15 < 16), 16 (80), 17 (81), 49 (113), 63 (127), 7 (< 16); N: 50, 1, 3, 16, 17, 139, 128, 64;
#   K: 70, 33 (% 32 = 1; 3 splits of 32: the third is EMPTY), 35 (3), 36 (4; 2 splits of 32: the second is SHORT), 37 (5),
#   63 (31), 31 and 5 (< 32; 9 splits of 32 over K = 5: eight empty), splits 1, 2, 3, 9.
GEMM_ROWS_16 = (
    (37, 50, 70, 1, dict(bias=True, relu=True)),
    (65, 1, 33, 3, {}),
    (15, 3, 35, 1, dict(bias=True)),
    (80, 16, 36, 2, {}),
    (81, 17, 37, 1, dict(relu=True, a_bf16=True)),
    (113, 139, 63, 1, dict(accumulate=True, b_bf16=True)),
    (127, 128, 31, 1, dict(bias=True, relu=True, accumulate=True)),
    (7, 64, 5, 9, {}),
    (37, 50, 70, 1, dict(round4=True)),                        # rows of 37 / 50 / 70 elements in strides of 40 / 52 / 72
    (37, 50, 70, 1, dict(round4=True, a_bf16=True, b_bf16=True)),
    (65, 33, 45, 1, dict(ldc_pad=3, bias=True)),
    (37, 50, 333, 1, dict(c_bf16=True, big=True, bias=True, relu=True)),
    (70, 33, 320, 1, dict(a_bf16=True, b_bf16=True, c_bf16=True, big=True)),
)
# 4 waves: at least 128 workgroups, with small K.  Tiles (M x N x splits): 17 x 8 = 136; 3 x 3 x 15 = 135 (K = 35: ranges 32, 3
# and thirteen empty); 1 x 15 x 9 = 135 (M = 7 < 16; K = 292: ranges of 64, the fifth SHORT (36), four empty); 17 x 1 x 9 = 153
# (K = 261: eight ranges of 32 and one of 5; K = 287: one of 31); 128 x 1 (M = 8177, % 64 = 49, K = 20 < 32); 64 x 1 x 2 = 128
# (M = 4095, % 64 = 63; K = 63: 32 + 31); 17 x 3 x 3 = 153 (K = 33: the third range EMPTY); 18 x 8 = 144.
GEMM_ROWS_4 = (
    (1025, 512, 33, 1, dict(bias=True, relu=True, accumulate=True)),
    (143, 139, 35, 15, {}),
    (7, 960, 292, 9, {}),
    (1040, 1, 261, 9, {}),
    (1041, 3, 287, 9, {}),
    (8177, 16, 20, 1, dict(bias=True)),
    (4095, 17, 63, 2, {}),
    (1025, 192, 33, 3, {}),
    (1025, 498, 70, 1, dict(round4=True)),                     # strides 1028 / 500 / 72
    (1025, 498, 70, 1, dict(round4=True, a_bf16=True, b_bf16=True)),
    (1089, 450, 36, 1, dict(ldc_pad=5, accumulate=True)),
    (1040, 512, 37, 1, dict(relu=True, a_bf16=True)),
    (1040, 512, 37, 1, dict(accumulate=True, b_bf16=True)),
    (1025, 512, 333, 1, dict(c_bf16=True, big=True, bias=True, relu=True)),
    (1041, 500, 320, 1, dict(a_bf16=True, b_bf16=True, c_bf16=True, big=True)),
)
TRANSPOSES = ((0, 0), (0, 1), (1, 0), (1, 1))
GEMM_CASES = tuple(GemmCase(w, M, N, K, ta, tb, ns, **opt) for w, rows in ((16, GEMM_ROWS_16), (4, GEMM_ROWS_4))
                   for M, N, K, ns, opt in rows for ta, tb in TRANSPOSES)
# one case per (ta, tb, template) between guard rows: the first row of each table without the accumulate
GEMM_GUARDED = tuple(c._replace(accumulate=False) for c in GEMM_CASES if (c.M, c.N, c.K) in ((37, 50, 70), (1025, 512, 33)) and c.bias)
# aligned rows against a pointer offset by one fp32 / two bf16 elements: the round4 rows (vector loads when aligned), each dtype
GEMM_OFFSET = tuple(c for c in GEMM_CASES if c.round4)


class GemmData(NamedTuple):
    A: torch.Tensor                              # as stored: (rows, lda) float32, NaN in the pad columns
    B: torch.Tensor
    bias: Optional[torch.Tensor]                 # (N,)
    target: Optional[torch.Tensor]               # (M, N): what C holds before an accumulating call
    slabs: Tuple[torch.Tensor, ...]              # fp64 (M, N) per K range; nsplit == 1: the finished output
    total: torch.Tensor                          # fp64 (M, N): the sum of the slabs


def gemm_ref(case: GemmCase, A, B, bias, target, drop_last_k=False, ignore_ld=False, ignore_trans_a=False):
    """The slabs of a case in fp64, stated from the ABI: opA(A)[m, k] = transA ? A[k * lda + m] : A[m * lda + k], likewise
    opB(B)[k, n].  The keyword arguments are the mutants of tests/test_gemm_exact_cpu.py."""
    M, N, K = case.M, case.N, case.K
    lda, ldb = (case.a_shape[1], case.b_shape[1]) if ignore_ld else (case.lda, case.ldb)
    fa, fb = A.double().flatten(), B.double().flatten()
    if ignore_trans_a:                           # A[m * lda + k] read from a transposed A (zeros past its end)
        fa = torch.cat([fa, torch.zeros(M * lda + K, dtype=torch.float64)])
    opA = torch.as_strided(fa, (M, K), (1, lda) if case.ta and not ignore_trans_a else (lda, 1))
    opB = torch.as_strided(fb, (K, N), (1, ldb) if case.tb else (ldb, 1))
    slabs = []
    for kbeg, kend in case.ranges:
        kend = min(kend, K - 1) if drop_last_k else kend
        slabs.append(opA[:, kbeg:max(kbeg, kend)] @ opB[kbeg:max(kbeg, kend)])
    if case.nsplit == 1:
        out = slabs[0]
        if bias is not None:
            out = out + bias.double()
        if case.relu:
            out = torch.relu(out)
        if target is not None:
            out = out + target.double()
        slabs = [out]
    return tuple(slabs)


@functools.lru_cache(maxsize=None)
def gemm_data(case: GemmCase) -> GemmData:
    """Operands and reference of a case, computed once; neither may be modified."""
    assert case.nsplit == 1 or not (case.bias or case.relu or case.c_bf16 or case.accumulate or case.ldc_pad)
    assert not (case.accumulate and case.c_bf16)
    M, N, K = case.M, case.N, case.K
    g = torch.Generator().manual_seed(M * 1000003 + N * 7919 + K * 31 + 2 * case.ta + case.tb + 5 * case.big)
    a, b = ints(g, M, K), ints(g, K, N)
    if case.big:                                 # every product a[m, k] * b[k, n] >= 0: a sign per k on magnitudes 0..2
        sign = torch.randint(0, 2, (K,), generator=g).float() * 2 - 1
        a, b = a.abs() * sign, b.abs() * sign[:, None]
    assert K * 2 * 2 + 2 + 2 < EXACT, "partial sums must stay exact in fp32"
    A = padded(a.t().contiguous() if case.ta else a, case.lda)
    B = padded(b.t().contiguous() if case.tb else b, case.ldb)
    if case.round4:
        assert all(row % 4 and ld % 4 == 0 and ld > row for row, ld in ((case.a_shape[1], case.lda), (case.b_shape[1], case.ldb)))
    bias = ints(g, N) if case.bias else None
    target = ints(g, M, N) if case.accumulate else None
    slabs = gemm_ref(case, A, B, bias, target)
    total = sum(slabs[1:], slabs[0])
    if case.c_bf16:
        assert bf16_ties(total) >= 1 and float(total.abs().max()) > 256, "a bf16-output case must round at least one tie"
    return GemmData(A, B, bias, target, slabs, total)


# ------------------------------------------------------------------------------------------------ grouped weight gradient
class Job(NamedTuple):
    M: int
    N: int
    K: int
    ldx: int
    x_bf16: bool
    bias: bool
    x_off: int = 0                               # X starts this many elements past an aligned address

    @property
    def wgs(self):                               # workgroups the job owns: the ones column may open a tile of its own
        return ceil_div(self.N, 64) * ceil_div(self.K + (1 if self.bias else 0), 64)


# At least 12 jobs (the kernel finds its job by binary search over the first-workgroup column), M in {1, 31, 32, 33, 97, 300},
# N in {3, 64, 65} (N % 4 != 0: dY on element loads), K in {64, 128} (with a bias the ones column n == K opens a tile of its
# own: 2 and 3 tiles), K % 64 == 63 (the ones column is the last of a tile), K % 4 in {1, 2, 3} (the ones column inside a
# partly valid group of four), each with and without a bias; ldx % 4 != 0, ldx > K, bf16 X, X off its alignment.  The first
# job, the last one and four others own exactly one workgroup.
JOBS = (
    Job(97, 3, 33, 36, False, True),             # 1 workgroup, K % 4 == 1, ldx > K
    Job(1, 3, 64, 64, False, True),              # 2
    Job(31, 64, 128, 128, False, True),          # 3
    Job(32, 65, 63, 64, True, True),             # 2 (N tiles), bf16 X
    Job(33, 3, 127, 127, False, True),           # 2, ldx % 4 != 0
    Job(300, 65, 34, 35, True, True),            # 2, K % 4 == 2, ldx % 4 != 0, bf16
    Job(97, 3, 35, 40, False, True, 1),          # 1, K % 4 == 3, X one float off
    Job(33, 64, 64, 64, False, False),           # 1
    Job(32, 3, 128, 132, True, False, 2),        # 2, bf16 X two elements off
    Job(31, 65, 63, 63, False, False),           # 2
    Job(1, 64, 33, 33, False, False),            # 1
    Job(300, 3, 34, 36, False, False),           # 1
    Job(97, 65, 35, 35, True, False),            # 2
    Job(300, 64, 127, 128, True, True),          # 2
    Job(31, 3, 3, 4, False, True),               # 1 workgroup: the last job
)


class JobData(NamedTuple):
    dy: torch.Tensor                             # (M, N)
    x: torch.Tensor                              # (M, ldx), NaN past column K
    dW: torch.Tensor                             # fp64 (N, K)
    db: Optional[torch.Tensor]                   # fp64 (N,)


def job_ref(job: Job, dy, x, ignore_ld=False, drop_last_k=False, ones_off=False, db_short=False):
    """(dW, db) in fp64: dW = dY^T X[:, :K], db = column sums of dY.  Keyword arguments: mutants."""
    M = job.M - 1 if drop_last_k else job.M      # (the contraction runs over the M rows)
    xs = torch.as_strided(x.double().flatten(), (job.M, job.K), (job.K if ignore_ld else job.ldx, 1))
    dW = dy.double()[:M].t() @ xs[:M]
    db = dy.double()[:job.M - 1 if db_short else job.M].sum(0) if job.bias else None
    if ones_off and job.bias:                    # the ones column at n == K - 1: its sums land in dW, db sees X's column K - 1
        dW, db = dW.clone(), dW[:, job.K - 1].clone()
        dW[:, job.K - 1] = dy.double().sum(0)
    return dW, db


@functools.lru_cache(maxsize=None)
def job_data(index: int) -> JobData:
    job = JOBS[index]
    g = torch.Generator().manual_seed(4001 + index)
    dy, x = ints(g, job.M, job.N), padded(ints(g, job.M, job.K), job.ldx)
    assert job.M * 2 * 2 < EXACT
    return JobData(dy, x, *job_ref(job, dy, x))


# ------------------------------------------------------------------------------------------------ FC chain, forward
FC_BATCH = 16 * 12                               # kFcBatch weight pieces of 16 k each: one trip of a wave


def chain_supported(K1, ldx, H, N2):
    """ka_fc_chain_supported restated."""
    T1 = H // 16
    ksplit = 1 if T1 >= 8 else (8 // T1 if T1 > 0 else 0)
    return (K1 >= 16 and K1 % 16 == 0 and K1 <= 2048 and ldx % 4 == 0 and ldx >= K1 and H >= 16 and H % 16 == 0 and H <= 512
            and (T1 >= 8 or T1 in (1, 2, 4)) and (K1 // ksplit) % 16 == 0 and N2 >= 1)


def chain_ksplit(H):
    return 1 if H // 16 >= 8 else 8 // (H // 16)


class ChainCase(NamedTuple):
    M: int
    K1: int
    ldx: int
    H: int
    N2: int
    b1: bool = True
    b2: bool = True
    affine: bool = False
    x_out: bool = False
    hidden_out: bool = True

    @property
    def id(self):
        flags = "".join(f"-{n}" for n in ("b1", "b2", "affine", "x_out", "hidden_out") if getattr(self, n))
        return f"M{self.M}-K{self.K1}.{self.ldx}-H{self.H}-N{self.N2}{flags}"

    @property
    def klen(self):                              # the K range of one phase-1 unit
        return self.K1 // chain_ksplit(self.H)


# H = 16, 32, 64: 8, 4, 2 K ranges per hidden tile (ksplit), smallest K1 = 16 * ksplit: 128, 64, 32; H = 128: ksplit 1, eight
# hidden tiles; H = 256, 512: 16 and 32 tiles, a wave owns more than one, and phase 2 (H > 192) takes two trips.  K range
# (K1 / ksplit) against one trip of 192: under (16 .. 128), equal (192; 384 / 2), over (208; 1664 / 8 = 208; 768).  N2 = 129
# and 139: 9 output tiles, wave 0 owns two.  M in {1, 15, 16, 17, 37}: one to three workgroups, the last one ragged.
CHAIN_CASES = (
    ChainCase(1, 128, 128, 16, 1),
    ChainCase(37, 1664, 1664, 16, 17, b1=False, affine=True, x_out=True),
    ChainCase(15, 64, 68, 32, 3, b2=False, affine=True, hidden_out=False),
    ChainCase(16, 32, 32, 64, 16, b1=False, b2=False),
    ChainCase(17, 384, 388, 64, 139, affine=True, x_out=True),
    ChainCase(17, 16, 16, 128, 17, hidden_out=False),
    ChainCase(37, 128, 384, 128, 129, affine=True),
    ChainCase(16, 192, 192, 128, 3, b1=False),
    ChainCase(15, 208, 208, 128, 16, b2=False, affine=True, x_out=True, hidden_out=False),
    ChainCase(37, 768, 1024, 128, 139),
    ChainCase(37, 192, 192, 256, 129, affine=True, x_out=True),
    ChainCase(1, 16, 20, 256, 1, b1=False, b2=False, hidden_out=False),
    ChainCase(17, 768, 768, 512, 139, affine=True, x_out=True),
)
CHAIN_GUARDED = ChainCase(37, 208, 212, 256, 139, affine=True, x_out=True)
ALPHA = 0.5


class ChainData(NamedTuple):
    x: torch.Tensor                              # (M, ldx), NaN past column K1
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    W1: torch.Tensor                             # (H, K1)
    b1: Optional[torch.Tensor]
    W2: torch.Tensor                             # (N2, H)
    b2: Optional[torch.Tensor]
    xp: torch.Tensor                             # fp64 (M, K1): x'
    hidden: torch.Tensor                         # fp64 (M, H)
    y: torch.Tensor                              # fp64 (M, N2)


def chain_ref(case: ChainCase, x, scale, shift, W1, b1, W2, b2, ignore_ld=False, drop_last_k=False):
    """(x', hidden, y) in fp64: x' = scale * (x * alpha) + shift or x; hidden = relu(x' W1^T + b1); y = hidden W2^T + b2."""
    xs = torch.as_strided(x.double().flatten(), (case.M, case.K1), (case.K1 if ignore_ld else case.ldx, 1))
    xp = scale.double() * (xs * ALPHA) + shift.double() if scale is not None else xs
    K = case.K1 - 1 if drop_last_k else case.K1
    hidden = xp[:, :K] @ W1.double()[:, :K].t()
    hidden = torch.relu(hidden + b1.double() if b1 is not None else hidden)
    y = hidden @ W2.double().t()
    return xp, hidden, y + b2.double() if b2 is not None else y


@functools.lru_cache(maxsize=None)
def chain_data(case: ChainCase) -> ChainData:
    assert chain_supported(case.K1, case.ldx, case.H, case.N2) and (case.affine or not case.x_out)
    g = torch.Generator().manual_seed(case.M + 13 * case.K1 + 101 * case.H + 1009 * case.N2)
    x = padded(ints(g, case.M, case.K1), case.ldx)
    scale = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (case.K1,), generator=g)] if case.affine else None
    shift = ints(g, case.K1) if case.affine else None
    xmax = 2 * (2 * ALPHA) + 2 if case.affine else 2                       # |x'|, a multiple of 0.5
    # the bound of y in units of 0.5 with weights in -2..2; where it would pass 2^23 the weights are in -1..1
    wmax = 2 if 2 * (case.H * (case.K1 * xmax * 2 + 2) * 2 + 2) < EXACT else 1
    hmax = case.K1 * xmax * wmax + 2
    assert 2 * (case.H * hmax * wmax + 2) < EXACT, "partial sums (multiples of 0.5) must stay exact in fp32"
    W1, W2 = ints(g, case.H, case.K1, lo=-wmax, hi=wmax), ints(g, case.N2, case.H, lo=-wmax, hi=wmax)
    b1 = ints(g, case.H) if case.b1 else None
    b2 = ints(g, case.N2) if case.b2 else None
    return ChainData(x, scale, shift, W1, b1, W2, b2, *chain_ref(case, x, scale, shift, W1, b1, W2, b2))


# ------------------------------------------------------------------------------------------------ FC chain, backward
class BwdCase(NamedTuple):
    M: int
    N2: int                                      # C: width of dy, the chain kernel's input
    H: int                                       # G: width of the saved hidden
    K1: int                                      # 3C: width of dx

    @property
    def id(self):
        return f"M{self.M}-C{self.N2}-G{self.H}-K{self.K1}"


# As _gpool_bwd calls it: N2 = C, H = G, K1 = 3 C.  The kernel runs as a forward chain of input width C, so C is the smallest
# multiple of 16 * ksplit(G): G = 16 -> C = 128, G = 32 -> 64, G = 64 -> 32, G = 128 and 256 (ksplit 1) -> 16 and 32; the last
# case has K1 = 50, no multiple of 16 (ragged output tiles).
BWD_CASES = (BwdCase(1, 128, 16, 384), BwdCase(15, 64, 32, 192), BwdCase(16, 32, 64, 96), BwdCase(17, 16, 128, 48),
             BwdCase(37, 32, 256, 96), BwdCase(37, 16, 128, 50))


class BwdData(NamedTuple):
    dy: torch.Tensor                             # (M, N2)
    hidden: torch.Tensor                         # (M, H): positives, +0.0 and -0.0
    W2: torch.Tensor                             # (N2, H), nn.Linear layout
    W1: torch.Tensor                             # (H, K1)
    dh: torch.Tensor                             # fp64 (M, H)
    dx: torch.Tensor                             # fp64 (M, K1)


def bwd_ref(dy, hidden, W2, W1, mask_ge=False, mask_from_new=False):
    """dh = (dy W2) * [hidden > 0], dx = dh W1 in fp64.  Keyword arguments: mutants."""
    pre = dy.double() @ W2.double()
    src = pre if mask_from_new else hidden.double()
    dh = pre * ((src >= 0) if mask_ge else (src > 0))
    return dh, dh @ W1.double()


@functools.lru_cache(maxsize=None)
def bwd_data(case: BwdCase) -> BwdData:
    assert chain_supported(case.N2, case.N2, case.H, case.K1)
    g = torch.Generator().manual_seed(case.M + 17 * case.N2 + 257 * case.H + case.K1)
    dy, W2, W1 = ints(g, case.M, case.N2), ints(g, case.N2, case.H), ints(g, case.H, case.K1)
    kind = torch.randint(0, 3, (case.M, case.H), generator=g)            # 0: positive, 1: +0.0, 2: -0.0
    hidden = torch.where(kind == 0, torch.randint(1, 4, (case.M, case.H), generator=g).float(), torch.zeros(()))
    hidden = torch.where(kind == 2, -hidden, hidden)
    assert bool((hidden > 0).any()) and bool(torch.signbit(hidden).any()) and bool(((hidden == 0) & ~torch.signbit(hidden)).any())
    assert case.H * (case.N2 * 4) * 2 < EXACT
    return BwdData(dy, hidden, W2, W1, *bwd_ref(dy, hidden, W2, W1))


# ------------------------------------------------------------------------------------------------ transposes
TRANSPOSE_SHAPES = ((1, 1), (1, 70), (31, 33), (32, 32), (33, 65), (256, 768))


def transpose_max_tiles(shapes):
    """max_tiles as _fc_transposed computes it: the most 32 x 32 tiles of any matrix of the table."""
    return max(ceil_div(r, 32) * ceil_div(c, 32) for r, c in shapes)


def transpose_swapped_stride(src):
    """The mutant: element (r, c) written to dst[c * C + r] instead of dst[c * R + r] (writes past the end dropped)."""
    R, C = src.shape
    dst = torch.zeros(R * C, dtype=src.dtype)
    r, c = torch.meshgrid(torch.arange(R), torch.arange(C), indexing="ij")
    idx = (c * C + r).flatten()
    keep = idx < R * C
    dst[idx[keep]] = src.flatten()[keep]
    return dst.reshape(C, R)


# ------------------------------------------------------------------------------------------------ column sums over row slices
# (M, nsplit, N): rows_per = ceil(M / nsplit) in {1, 3, 4, 5, 28, 29, 32, 33, 36, 37}.  A workgroup's four 64-lane groups take
# rows mbeg + sl, + 4, ...; the unrolled loop (eight rows in flight) runs while m + 28 < mend: group 0 enters it from 29 rows,
# group 3 from 32, a second trip would need 61; 28 and 29, 32 and 33, 36 and 37 sit on both sides of those edges and of a
# fourfold row count.  (5, 7): more slices than rows, slices 5 and 6 are empty.  Last slices are short wherever M % nsplit != 0.
SLICE_CASES = ((5, 5, 1), (5, 7, 63), (8, 3, 64), (11, 3, 65), (14, 3, 139), (55, 2, 1), (57, 2, 63), (95, 3, 64), (65, 2, 65),
               (71, 2, 139), (110, 3, 65))


def slice_rows(M, nsplit):
    rp = ceil_div(M, nsplit)
    return rp, [(min(M, z * rp), min(M, (z + 1) * rp)) for z in range(nsplit)]


def slice_sums(t, M, nsplit, short=False):
    """(nsplit, N) fp64: the column sums of each row slice of t (M, N); short: the mutant that stops one row early."""
    return torch.stack([t.double()[b:max(b, e - (1 if short else 0))].sum(0) for b, e in slice_rows(M, nsplit)[1]])


@functools.lru_cache(maxsize=None)
def slice_data(M, nsplit, N):
    """(A, Bm, mean, invstd): integers; the mean is an integer and invstd a power of two, so (Bm - mean) * invstd is exact."""
    g = torch.Generator().manual_seed(M * 131 + nsplit * 17 + N)
    A, Bm, mean = ints(g, M, N), ints(g, M, N), ints(g, N)
    invstd = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N,), generator=g)]
    assert M * 2 * (4 * 2) < EXACT
    return A, Bm, mean, invstd


REDUCE_SPLITS = (1, 7, 8, 9, 17)                 # the eight-at-a-time loop: not entered, one short of it, exactly, one over, 2 x 8 + 1
REDUCE_SIZES = (1, 255, 257)
GRID_STRIDE_ROWS, GRID_STRIDE_COLS = 8200, 139   # 1 139 800 elements > 4096 * 256: every grid-stride loop of the file iterates


# ------------------------------------------------------------------------------------------------ mutants of the references
# Each is a reference with one of the mistakes such a kernel can make (the keyword arguments of the *_ref functions above), as
# a predicate "the mutant passes torch.equal on this case", with the cases the mistake applies to.
ALL_CHAIN = CHAIN_CASES + (CHAIN_GUARDED,)


def same(a, b):
    """torch.equal on tuples of optional tensors (NaN never equal: an unwritten slab fails)."""
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def gemm_mutant(**kw):
    return lambda c: same(gemm_ref(c, *gemm_data(c)[:4], **kw), gemm_data(c).slabs)


def unwritten_empty_split(c):
    d = gemm_data(c)
    return same([torch.full_like(s, float("nan")) if b == e else s for (b, e), s in zip(c.ranges, d.slabs)], d.slabs)


def bf16_truncation(c):
    total = gemm_data(c).total
    return torch.equal(bf16_truncated(total), total.float().bfloat16())


def job_mutant(**kw):
    return lambda i: same(job_ref(JOBS[i], job_data(i).dy, job_data(i).x, **kw), job_data(i)[2:])


def chain_mutant(**kw):
    return lambda c: same(chain_ref(c, *chain_data(c)[:7], **kw)[1:], chain_data(c)[8:])


def bwd_mutant(**kw):
    return lambda c: same(bwd_ref(*bwd_data(c)[:4], **kw), bwd_data(c)[4:])


def slice_short(case):
    M, ns, N = case
    A = slice_data(M, ns, N)[0]
    return torch.equal(slice_sums(A, M, ns, short=True), slice_sums(A, M, ns))


def transpose_stride(shape):
    src = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[0] * 1000 + shape[1]))
    return torch.equal(transpose_swapped_stride(src), src.t())


JOB_IDX = tuple(range(len(JOBS)))
# name -> [(passes(case) -> bool, the cases the mistake applies to)]
MUTANTS = {
    "last_k_dropped": [(gemm_mutant(drop_last_k=True), GEMM_CASES), (job_mutant(drop_last_k=True), JOB_IDX),
                       (chain_mutant(drop_last_k=True), ALL_CHAIN)],
    "ld_ignored": [(gemm_mutant(ignore_ld=True), tuple(c for c in GEMM_CASES if c.round4)),
                   (job_mutant(ignore_ld=True), tuple(i for i in JOB_IDX if JOBS[i].ldx > JOBS[i].K and JOBS[i].M > 1)),
                   (chain_mutant(ignore_ld=True), tuple(c for c in ALL_CHAIN if c.ldx > c.K1 and c.M > 1))],
    "trans_a_ignored": [(gemm_mutant(ignore_trans_a=True), tuple(c for c in GEMM_CASES if c.ta))],
    "empty_split_unwritten": [(unwritten_empty_split, tuple(c for c in GEMM_CASES if any(b == e for b, e in c.ranges)))],
    # (one row whose last X element is 1: column K - 1 of X IS a column of ones, the mistake changes nothing)
    "ones_column_off_by_one": [(job_mutant(ones_off=True), tuple(i for i in JOB_IDX if JOBS[i].bias and JOBS[i].M > 1))],
    "bias_gradient_one_row_short": [(job_mutant(db_short=True), tuple(i for i in JOB_IDX if JOBS[i].bias))],
    "relu_mask_ge": [(bwd_mutant(mask_ge=True), BWD_CASES)],
    "mask_from_new_preactivation": [(bwd_mutant(mask_from_new=True), BWD_CASES)],
    "bf16_truncated": [(bf16_truncation, tuple(c for c in GEMM_CASES if c.c_bf16))],
    "slice_one_row_short": [(slice_short, SLICE_CASES)],
    "transpose_stride_swapped": [(transpose_stride, tuple(s for s in TRANSPOSE_SHAPES if s[0] != s[1]))],
}
