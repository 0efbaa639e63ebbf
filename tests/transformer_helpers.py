"""Shared by tests/test_transformer_exact_cpu.py and tests/test_hip_transformer_exact.py: operands, fp64 references stated from
the C ABI comments of csrc/transformer.hip, restatements of its launch rules, the mutants of the references, and the case lists.

Why integers: the GEMMs multiply bf16 operands on the matrix cores with fp32 accumulation.  With operands in -2..2 every product
is exact and every partial sum an integer far below 2^24, so fp32 addition is exact in ANY order; bias, residual, the ReLU masks
and a dropout at p = 0.5 (kept scale exactly 2) keep the values integers, and the operands are sparse enough where K is large
that every bf16 output is exactly representable.  The result must equal the fp64 reference to the bit whatever the kernel form,
tile map, split or store path, and one dropped, doubled or misplaced element changes it.  The attention kernels get the same
treatment through a one-hot softmax (below), LayerNorm and the random-operand attention cases bounds derived from the formats."""
import functools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from gemm_helpers import NAN, ceil_div, ints, padded

EXACT = 2 ** 24                                  # every |partial sum| stays below this
SEED_BIG = (0x1234 << 32) | 0x9ABCDEF1           # a seed above 2^32: the high word enters the key
SEED_SMALL = 424242


# ------------------------------------------------------------------------------------------------ the dropout mask
def _hash32(x):
    """hash32 of csrc/transformer.hip on uint64 arrays holding 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def drop_thresh(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5)) if p > 0 else 0


def inv_keep(p):
    """1 / (1 - p) as the kernels compute it, in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def keep_at(seed, index, p):
    """The keep decision of (seed, element index) for an int64 tensor of indices, from the rule at the top of transformer.hip:
    threshold uint32(p * 65536 + 0.5); key = lo32(seed) * 0x9E3779B1 + hi32(seed) * 0x85EBCA6B; pair = index >> 1;
    h = hash32(lo32(pair) * 0x9E3779B1 + hi32(pair) * 0xC2B2AE35 + key); kept iff the 16-bit half of h (low: even index,
    high: odd index) is at or above the threshold.  Plain integer numpy, all arithmetic modulo 2^32."""
    m = np.uint64(0xFFFFFFFF)
    idx = index.numpy().astype(np.uint64)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    key = ((lo * np.uint64(0x9E3779B1)) & m) + ((hi * np.uint64(0x85EBCA6B)) & m) & m
    pair = idx >> np.uint64(1)
    x = (((pair & m) * np.uint64(0x9E3779B1)) & m) + (((pair >> np.uint64(32)) * np.uint64(0xC2B2AE35)) & m) + (key & m)
    h = _hash32(x & m)
    bits = np.where(idx & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return torch.from_numpy(bits >= np.uint64(drop_thresh(p)))


def keep_mask(seed, n, p):
    """(n,) bool: element i of a tensor of n elements is kept."""
    return keep_at(seed, torch.arange(n, dtype=torch.int64), p)


DROP_PS = (0.0, 0.1, 0.3, 0.5)
DROP_NS = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 81 * 24 + 1)


def zeros_and_signs(g, *shape):
    """Integers in -2..2 in which both +0.0 and -0.0 occur (a ReLU mask 'keep iff > 0' drops both)."""
    t = torch.randint(-2, 3, shape, generator=g).float()
    neg = torch.randint(0, 2, shape, generator=g).bool()
    return torch.where((t == 0) & neg, torch.tensor(-0.0), t)


# ------------------------------------------------------------------------------------------------ NT GEMM
K_TILE, BM, BN = 64, 128, 128
EPILOGUES = ("none", "bias", "bias_relu", "bias_relu_drop", "bias_drop_res", "res", "masked0", "masked5")
MASKED = ("masked0", "masked5")


def nt_len(K, nsplit):
    """K range of one slab as ka_tf_gemm_nt cuts it: whole 64-steps."""
    return K if nsplit <= 1 else ceil_div(ceil_div(K, K_TILE), nsplit) * K_TILE


def nt_slabs(K, nsplit):
    """ka_tf_gemm_nt_slabs restated."""
    return 1 if nsplit <= 1 else ceil_div(K, nt_len(K, nsplit))


def nt_ranges(K, nsplit):
    ln = nt_len(K, nsplit)
    return [(s * ln, min(K, (s + 1) * ln)) for s in range(nt_slabs(K, nsplit))]


class NtCase(NamedTuple):
    form: str                                    # the route the case claims: tiled | k256 | big | map
    M: int
    N: int
    K: int
    epi: str = "none"
    c_bf16: bool = False
    lda_pad: int = 0
    ldb_pad: int = 0
    ldc_pad: int = 0
    nsplit: int = 1

    @property
    def id(self):
        return (f"{self.form}-{self.M}x{self.N}x{self.K}-{self.epi}-{'bf16' if self.c_bf16 else 'f32'}"
                f"-ld+{self.lda_pad}+{self.ldb_pad}+{self.ldc_pad}" + (f"-s{self.nsplit}" if self.nsplit > 1 else ""))

    @property
    def lda(self):
        return self.K + self.lda_pad

    @property
    def ldb(self):
        return self.K + self.ldb_pad

    @property
    def ldc(self):
        return self.N + self.ldc_pad

    @property
    def p(self):
        return 0.5 if self.epi in ("bias_relu_drop", "bias_drop_res", "masked5") else 0.0

    @property
    def masked(self):
        return self.epi in MASKED

    @property
    def ranges(self):
        return nt_ranges(self.K, self.nsplit)


def nt_route(c: NtCase, k256=True, big=True):
    """The form tf_gemm_nt_impl launches, restated: K = 256 activation-stationary, the 256 x 256 tile form, or the tiled
    kernel ('map' when its grid is walked as 8 x 8 super-tiles)."""
    one = nt_slabs(c.K, c.nsplit) == 1
    res, act = c.epi in ("bias_drop_res", "res"), c.masked
    if k256 and c.K == 256 and one and c.c_bf16 and c.N % 64 == 0 and c.N <= 4096 and c.ldc % 8 == 0:
        return "k256"
    if (big and one and c.M >= 1024 and c.N >= 1024 and c.K >= 1024 and c.K % 64 == 0 and not res and not act
            and c.epi in ("none", "bias")):
        return "big"
    return "map" if ceil_div(c.N, BN) > 8 and ceil_div(c.M, BM) >= 8 else "tiled"


def nt_lds_epilogue(c: NtCase):
    """Has a tile that leaves through LDS (the counter KA_TF_LDS_EPI switches): full bf16 tiles, N and ldc multiples of 8."""
    return nt_slabs(c.K, c.nsplit) == 1 and c.c_bf16 and c.N % 8 == 0 and c.ldc % 8 == 0 and c.M >= BM and c.N >= BN


def _cycle(seq, i):
    return seq[i % len(seq)]


def _tiled_cases():
    """N x epilogue x output type, the other axes cycled so that every value of every axis occurs: M in {1, 127, 128, 129,
    257}, K in {32, 64, 96, 2592}, lda / ldb in {K, K + 8}, ldc in {N, N + 1, N + 4, N + 8}; every dropout case at two ldc."""
    Ms, Ks, Ns = (1, 127, 128, 129, 257), (32, 64, 96, 2592), (1, 3, 4, 7, 8, 127, 128, 136, 139)
    pads, out, i = (0, 1, 4, 8), [], 0
    for c_bf16 in (False, True):
        for epi in EPILOGUES:
            if epi in MASKED and not c_bf16:
                continue
            for N in Ns:
                M, K = _cycle(Ms, i), _cycle(Ks, i // 2 + i // 7)
                base = NtCase("tiled", M, N, K, epi, c_bf16, 8 * (i % 2), 8 * (i // 2 % 2), _cycle(pads, i))
                out.append(base)
                if base.p:
                    out.append(base._replace(ldc_pad=_cycle(pads, i + 1 + i // 4 % 3)))
                i += 1
    return tuple(out)


NT_TILED = _tiled_cases()
# full and ragged tiles together, eligible for the LDS epilogue: every bf16 epilogue with the switch on and off
NT_LDS = tuple(NtCase("tiled", M, N, K, epi, True, 8, 0, pad) for epi, (M, N, K, pad) in
               zip(EPILOGUES, ((257, 136, 96, 0), (129, 128, 64, 8), (257, 136, 32, 8), (128, 136, 96, 0), (257, 128, 64, 8),
                               (129, 136, 96, 0), (257, 136, 64, 8), (257, 136, 96, 0))))
# (nsplit, K) -> slabs: (2, 96) 2, the last one short (32); (2, 64) 1 < 2; (3, 160) 3, last 32; (3, 256) 2 < 3; (8, 576) 5 < 8,
# last 64 of 128; (8, 2592) 7 < 8, last 288 of 384
NT_SPLIT = tuple(NtCase("tiled", M, N, K, nsplit=ns, lda_pad=la, ldb_pad=lb, ldc_pad=lc) for M, N, K, ns, la, lb, lc in
                 ((129, 139, 96, 2, 0, 8, 0), (130, 8, 64, 2, 8, 0, 4), (127, 136, 160, 3, 0, 0, 1), (257, 7, 256, 3, 8, 8, 0),
                  (128, 128, 576, 8, 0, 8, 8), (65, 139, 2592, 8, 8, 0, 0)))
# gx = 9 > 8 n-tiles and gy = 8 m-tiles: the smallest shape on the super-tile map
NT_MAP = (NtCase("map", 897, 1025, 64, "bias_relu", True, 0, 8, 7), NtCase("map", 897, 1025, 64, "none", False, 8, 0, 0))


def _k256_cases():
    epis = ("none", "bias_relu_drop", "bias_drop_res", "masked5", "res", "masked0")      # (RES, ACT) = 00, 00, 10, 01, 10, 01
    out, i = [], 0
    for M in (1, 127, 128, 129, 300):
        for N in (64, 128, 272, 1024):
            c = NtCase("k256", M, N, 256, _cycle(epis, i), True, 8 * (i % 2), 8 * (i // 2 % 2), 8 * (i // 3 % 2))
            out.append(c._replace(form=nt_route(c)))
            i += 1
    return tuple(out)


NT_K256 = _k256_cases()
NT_BIG = (NtCase("big", 1024, 1024, 1024, "bias", False), NtCase("big", 1024, 1024, 1024, "none", True),
          NtCase("big", 1025, 1027, 1088, "bias", False, 8, 0, 1), NtCase("big", 1025, 1027, 1088, "none", True, 0, 8, 5),
          NtCase("big", 1281, 2305, 1024, "bias", False, 0, 8, 0), NtCase("big", 1281, 2305, 1024, "none", True, 8, 0, 7),
          NtCase("map", 1024, 1152, 1056, "bias", False), NtCase("map", 1024, 1152, 1056, "none", True, 0, 0, 8))
NT_CASES = NT_TILED + NT_LDS + NT_SPLIT + NT_MAP + NT_K256 + NT_BIG


class NtData(NamedTuple):
    A: torch.Tensor                              # (M, lda) float32, NaN past column K
    B: torch.Tensor                              # (N, ldb)
    bias: Optional[torch.Tensor]                 # (N,)
    res: Optional[torch.Tensor]                  # (M, ldc), NaN past column N
    act: Optional[torch.Tensor]                  # (M, ldc): positives, negatives, +0.0 and -0.0
    seed: int
    slabs: Tuple[torch.Tensor, ...]              # fp64 (M, N) per K range; one slab: the finished output


def nt_ref(c: NtCase, A, B, bias, res, act, seed, drop_last_ktile=False, mask_ld_n=False, res_before_drop=False, act_ge=False,
           neighbour_slab=False):
    """The slabs in fp64 from the ABI: C = epilogue(A[:, :K] B[:, :K]^T); the epilogue is bias, ReLU, dropout keep(seed,
    row * ldc + col) / (1 - p), the activation mask [relu_act > 0], then the residual.  Keyword arguments: the mutants."""
    a, b = A[:, :c.K].double(), B[:, :c.K].double()
    slabs = []
    for s, (kb, ke) in enumerate(c.ranges):
        if drop_last_ktile and ke == c.K:
            ke = (c.K - 1) // K_TILE * K_TILE
        if neighbour_slab and len(c.ranges) > 1:           # the first column of the next range counted here, not there
            kb, ke = kb + (1 if s > 0 else 0), ke + (1 if s + 1 < len(c.ranges) else 0)
        slabs.append(a[:, kb:max(kb, ke)] @ b[:, kb:max(kb, ke)].t())
    if len(slabs) > 1:
        return tuple(slabs)
    v = slabs[0]
    if bias is not None:
        v = v + bias.double()
    if "relu" in c.epi:
        v = torch.relu(v)
    if res is not None and res_before_drop:
        v = v + res[:, :c.N].double()
    if c.p:
        row, col = torch.meshgrid(torch.arange(c.M), torch.arange(c.N), indexing="ij")
        v = torch.where(keep_at(seed, row * (c.N if mask_ld_n else c.ldc) + col, c.p), v * 2.0, torch.zeros(()).double())
    if act is not None:
        a_ = act[:, :c.N]
        v = torch.where((a_ >= 0) if act_ge else (a_ > 0), v, torch.zeros(()).double())
    if res is not None and not res_before_drop:
        v = v + res[:, :c.N].double()
    return (v,)


def _nt_operands(c: NtCase, attempt=0):
    """The operands depend on (M, N, K, epilogue) only: the same products at every ld, form and split."""
    g = torch.Generator().manual_seed(c.M * 1000003 + c.N * 7919 + c.K * 31 + EPILOGUES.index(c.epi) + 104729 * attempt)
    a = ints(g, c.M, c.K)
    if c.K > 48:                                 # about 48 non-zero products per output: every result fits bf16
        a = a * (torch.rand(c.M, c.K, generator=g) < 48.0 / c.K)
        a[:, -1] = torch.where(a[:, -1] == 0, torch.ones(()), a[:, -1])
        a[:, (c.K - 1) // K_TILE * K_TILE] = 1.0             # something in the last k-tile besides its last column
    b = ints(g, c.N, c.K, lo=-1, hi=1) if c.K >= 1024 else ints(g, c.N, c.K)
    bias = ints(g, c.N) if "bias" in c.epi else None
    res = ints(g, c.M, c.N) if "res" in c.epi else None
    act = zeros_and_signs(g, c.M, c.N) if c.masked else None
    return a, b, bias, res, act


@functools.lru_cache(maxsize=None)
def nt_data(c: NtCase) -> NtData:
    """Operands and reference of a case, computed once; neither may be modified."""
    seed = SEED_BIG if (c.M + c.N) % 2 else SEED_SMALL
    for attempt in range(16):                    # redrawn until a dropped last k-tile shows: a ReLU, a mask or a dropout can hide it in a 1 x 1 output
        a, b, bias, res, act = _nt_operands(c, attempt)
        A, B = padded(a, c.lda), padded(b, c.ldb)
        res = None if res is None else padded(res, c.ldc)
        act = None if act is None else padded(act, c.ldc)
        slabs = nt_ref(c, A, B, bias, res, act, seed + attempt)
        if not same(slabs, nt_ref(c, A, B, bias, res, act, seed + attempt, drop_last_ktile=True)):
            return NtData(A, B, bias, res, act, seed + attempt, slabs)
    raise AssertionError(f"{c.id}: no operands found")


def nt_partial_bound(c: NtCase, d: NtData):
    """The largest |partial sum| any summation order can reach: sum_k |a| |b|, plus the epilogue's terms, doubled."""
    return float((d.A[:, :c.K].abs().double() @ d.B[:, :c.K].abs().double().t()).max()) * 2 + 8


# ------------------------------------------------------------------------------------------------ TN GEMM
TN_ROWS = 64


def tn_len(M, nsplit):
    return M if tn_slabs(M, nsplit) == 1 else ceil_div(ceil_div(M, TN_ROWS), nsplit) * TN_ROWS


def tn_slabs(M, nsplit):
    """ka_tf_gemm_tn_slabs restated: token ranges of whole 64-row steps."""
    if nsplit <= 1:
        return 1
    return ceil_div(M, ceil_div(ceil_div(M, TN_ROWS), nsplit) * TN_ROWS)


def tn_ranges(M, nsplit):
    ln = tn_len(M, nsplit)
    return [(z * ln, min(M, (z + 1) * ln)) for z in range(tn_slabs(M, nsplit))]


class TnCase(NamedTuple):
    M: int
    N: int
    K: int
    nsplit: int
    slabs: int                                   # what ka_tf_gemm_tn_slabs must answer
    lda_pad: int = 0
    ldb_pad: int = 0
    ldc_pad: int = 0

    @property
    def id(self):
        return f"{self.M}x{self.N}x{self.K}-s{self.nsplit}.{self.slabs}-ld+{self.lda_pad}+{self.ldb_pad}+{self.ldc_pad}"

    @property
    def lda(self):
        return self.N + self.lda_pad

    @property
    def ldb(self):
        return self.K + self.ldb_pad

    @property
    def ldc(self):
        return self.K + self.ldc_pad

    @property
    def ranges(self):
        return tn_ranges(self.M, self.nsplit)


# slab counts 1, 2, 7, 8, 9, 16, 17 on N = K = 8 with M one row past 64 * (slabs - 1): the XCD remap of the kernel acts on whole
# groups of 8 slabs (8: all remapped; 9: eight remapped and one not; 16, 17 likewise; 7: none); then M in {1, 63, 64, 65, 4097}
# and N, K in {8, 120, 128, 136, 264} (one, two and three tiles; K > 128: more than one k-tile beside the column sums), operand
# rows wider than N / K, ldc = K (vec4), K + 4 (vec4), K + 1 (scalar stores).
TN_CASES = tuple(TnCase(64 * (s - 1) + 1, 8, 8, s, s, 8 * (s % 2), 8 * (s // 2 % 2), (0, 4, 1)[s % 3]) for s in (1, 2, 7, 8, 9, 16, 17)) + (
    TnCase(1, 120, 264, 1, 1, 8, 0, 1), TnCase(63, 128, 136, 1, 1, 0, 8, 4), TnCase(64, 136, 128, 2, 1, 8, 8, 0),
    TnCase(65, 264, 120, 2, 2, 0, 0, 1), TnCase(4097, 136, 264, 4, 4, 8, 0, 4), TnCase(4097, 8, 120, 16, 13, 0, 8, 0),
    TnCase(65, 264, 264, 1, 1, 8, 8, 1), TnCase(200, 120, 136, 3, 2, 0, 0, 0))


class TnData(NamedTuple):
    A: torch.Tensor                              # (M, lda), NaN past column N
    B: torch.Tensor                              # (M, ldb), NaN past column K
    slabs: torch.Tensor                          # fp64 (slabs, N, K)
    colsum: torch.Tensor                         # fp64 (slabs, N)


def tn_ref(c: TnCase, A, B, neighbour_slab=False, drop_last_row=False):
    """C[z] = A[rows of z, :N]^T B[rows of z, :K], colsum[z] = column sums of A over the same rows, in fp64."""
    a, b = A[:, :c.N].double(), B[:, :c.K].double()
    C, cs = [], []
    for z, (mb, me) in enumerate(c.ranges):
        if neighbour_slab and len(c.ranges) > 1:
            mb, me = mb + (1 if z > 0 else 0), me + (1 if z + 1 < len(c.ranges) else 0)
        if drop_last_row and me == c.M:
            me -= 1
        C.append(a[mb:me].t() @ b[mb:me]); cs.append(a[mb:me].sum(0))
    return torch.stack(C), torch.stack(cs)


@functools.lru_cache(maxsize=None)
def tn_data(c: TnCase) -> TnData:
    g = torch.Generator().manual_seed(c.M * 1009 + c.N * 31 + c.K)
    a, b = ints(g, c.M, c.N), ints(g, c.M, c.K)
    a[a == 0] = 1.0                              # (a row that carries nothing would hide its own misplacement)
    assert c.M * 4 < EXACT
    A, B = padded(a, c.lda), padded(b, c.ldb)
    return TnData(A, B, *tn_ref(c, A, B))


# ------------------------------------------------------------------------------------------------ attention, one-hot
S, SP = 81, 96                                   # squares; the padded extent of the dropout index


def attn_register_form(bf16, H, dh, B=1, lds_switch=False):
    """The register-resident kernels take bf16 with dh <= 32, dh % 8 == 0 (restated from ka_tf_attention_fwd)."""
    return bf16 and dh <= 32 and dh % 8 == 0 and (H * dh) % 8 == 0 and B * H * SP * SP < 2 ** 32 and not lds_switch


class HotCase(NamedTuple):
    B: int
    H: int
    dh: int

    @property
    def id(self):
        return f"B{self.B}-H{self.H}-dh{self.dh}"

    @property
    def c(self):                                 # the magnitude of the key entries
        return 16 if self.dh <= 16 else 32

    @property
    def weights(self):
        """(dh,) the factor of each query dimension: 1 on the first 2^(k+1) - dh dimensions and 1/2 on the others, 2^k the
        largest power of two <= dh (all 1 where dh is one).  The selected score sum_i w_i c^2 = 2^k c^2 is then a power of
        two whatever dh is, so its product with the fp32 scale 1 / sqrt(dh) is exact.  Without that (dh = 24, 40, 56 with equal
        weights) the forward stores lse = fl(s scale) and the backward forms fma(s, scale, -lse) != 0: P = exp(2e-4), not 1,
        and dQ, dK come out as rounding noise of scores near 8000 instead of exact zeros -- fp32, not a defect."""
        pow2 = 1 << (self.dh.bit_length() - 1)
        ones = 2 * pow2 - self.dh
        assert ones >= 8                         # (the first 8 dimensions carry the signs that make the keys distinct)
        return torch.cat([torch.ones(ones), torch.full((self.dh - ones,), 0.5)])


# B * H = 1 (three surplus waves), 3 and 10 (remainders 3 and 2), 9 and 5 (remainder 1), 8 (none; H = 8 has no other remainder);
# dh = 24: half-filled second tile; 40, 48, 56, 64: the LDS kernels with three and four tiles.
HOT_CASES = (HotCase(1, 1, 8), HotCase(5, 1, 8), HotCase(1, 3, 16), HotCase(3, 3, 16), HotCase(2, 5, 24), HotCase(1, 8, 32),
             HotCase(1, 3, 40), HotCase(1, 2, 48), HotCase(2, 1, 56), HotCase(1, 2, 64))


class HotData(NamedTuple):
    qkv: torch.Tensor                            # (B * 81, 3 d) float32, exactly representable in bf16
    dout: torch.Tensor                           # (B * 81, d) integers
    phi: torch.Tensor                            # (B, H, 81) int64: the key every query selects
    smax: float                                  # the selected score before scaling: c^2 sum(w), a power of two


@functools.lru_cache(maxsize=None)
def hot_data(case: HotCase, many_to_one: bool) -> HotData:
    """Per (board, head): 81 distinct sign vectors +-c as keys, q_s = w * k_phi(s) (w: HotCase.weights) for a permutation or a
    many-to-one map phi drawn anew, integer V and dout.  The selected score c^2 sum(w) beats every other by at least c^2, after
    scaling by more than 120: exp underflows to exactly 0 in fp32 and the softmax is one-hot."""
    B, H, dh, c = case.B, case.H, case.dh, case.c
    g = torch.Generator().manual_seed(B * 100 + H * 10 + dh + (7 if many_to_one else 0))
    q = torch.empty(B, S, H, dh); k = torch.empty(B, S, H, dh)
    phi = torch.empty(B, H, S, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            code = torch.randperm(256, generator=g)[:S]                              # distinct in their first 8 signs
            sign = torch.randint(0, 2, (S, dh), generator=g)
            sign[:, :8] = (code[:, None] >> torch.arange(8)) & 1
            keys = (sign.float() * 2 - 1) * c
            ph = torch.randint(0, S, (S,), generator=g) if many_to_one else torch.randperm(S, generator=g)
            if many_to_one:
                ph[0], ph[80] = 80, 80                                                 # the last key is used, more than once
            k[b, :, h], q[b, :, h], phi[b, h] = keys, keys[ph] * case.weights, ph
    v = torch.randint(-2, 3, (B, S, H, dh), generator=g).float()
    v[v == 0] = 1.0                              # (a zero would hide which row was read)
    v = v + torch.arange(H).float()[None, None, :, None] * (v > 0)                   # heads differ: positives of head h are 1 + h, 2 + h
    dout = torch.randint(-2, 3, (B, S, H, dh), generator=g).float()
    dout[dout == 0] = -1.0
    d = H * dh
    qkv = torch.cat([q.reshape(B * S, d), k.reshape(B * S, d), v.reshape(B * S, d)], 1).contiguous()
    return HotData(qkv, dout.reshape(B * S, d).contiguous(), phi, float(c * c * case.weights.sum()))


def hot_scores(case: HotCase, d: HotData):
    """(B, H, 81, 81) fp64: q k^T, unscaled."""
    dm = case.H * case.dh
    q, k = (t.reshape(case.B, S, case.H, case.dh).transpose(1, 2).double() for t in (d.qkv[:, :dm], d.qkv[:, dm:2 * dm]))
    return q @ k.transpose(-1, -2)


def hot_keep(case: HotCase, d: HotData, seed, p):
    """(B, H, 81) fp64: the factor dropout puts on the one probability of each row: keep at ((b H + h) 96 + s) 96 + phi(s)."""
    bh = torch.arange(case.B * case.H).reshape(case.B, case.H, 1)
    idx = (bh * SP + torch.arange(S)) * SP + d.phi
    return keep_at(seed, idx, p).double() * inv_keep(p) if p else torch.ones(case.B, case.H, S, dtype=torch.float64)


def hot_ref(case: HotCase, d: HotData, seed=0, p=0.0, drop_key_80=False, next_head_v=False, no_surplus_repeat=False, dv_last_only=False):
    """(out (B*81, d), dV (B*81, d)) in fp64: out[b, s, h] = f V[b, phi(s), h], dV[b, t, h] = sum over phi(s) = t of f dout[b, s, h]
    with f the dropout factor of row s.  Keyword arguments: the mutants."""
    B, H, dh, dm = case.B, case.H, case.dh, case.H * case.dh
    v = d.qkv[:, 2 * dm:].reshape(B, S, H, dh).double()
    do = d.dout.reshape(B, S, H, dh).double()
    f = hot_keep(case, d, seed, p)
    out, dv = torch.zeros(B, S, H, dh, dtype=torch.float64), torch.zeros(B, S, H, dh, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            ph, fs = d.phi[b, h], f[b, h].clone()
            if drop_key_80:                      # the last key column never read: its queries see nothing
                fs = fs * (ph != 80)
            vh = v[b, :, (h + 1) % H if next_head_v else h]
            out[b, :, h] = fs[:, None] * vh[ph]
            if dv_last_only:                     # a store instead of a sum: the last query of each key wins
                dv[b, ph, h] = fs[:, None] * do[b, :, h]
            else:
                dv[b, :, h].index_add_(0, ph, fs[:, None] * do[b, :, h])
    if no_surplus_repeat:                        # the workgroup that has surplus waves never runs: its pairs stay unwritten
        for bh in range(B * H // 4 * 4, B * H):
            out[bh // H, :, bh % H] = NAN
    return out.reshape(B * S, dm), dv.reshape(B * S, dm)


# ------------------------------------------------------------------------------------------------ attention, fp64 oracle
def bf16r(t):
    """Rounded once to bf16, kept in fp64."""
    return t.float().bfloat16().double()


def attn_ref64(qkv, dout, B, H, dh, emulate=False, d_from_out=False):
    """(out, lse, dq, dk, dv) of softmax(Q K^T / sqrt(dh)) V per (board, head) in fp64, shapes (B, H, 81, .).  emulate: bf16
    storage where the kernels place it -- P before P V, dS and P before their products, each output rounded once; d_from_out:
    D = rowsum(dO O) from the rounded output (ka_tf_attention_bwd_o) instead of rowsum(dP P)."""
    r = bf16r if emulate else (lambda t: t)
    d = H * dh
    q, k, v = (t.reshape(B, S, H, dh).transpose(1, 2).double() for t in (qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]))
    do = dout.reshape(B, S, H, dh).transpose(1, 2).double()
    scale = 1.0 / math.sqrt(dh)
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = r(r(p) @ v)
    dp = do @ v.transpose(-1, -2)
    D = (do * out).sum(-1, keepdim=True) if d_from_out else (dp * p).sum(-1, keepdim=True)
    ds = r(p * (dp - D) * scale)
    return out, lse, r(ds @ k), r(ds.transpose(-1, -2) @ q), r(r(p).transpose(-1, -2) @ do)


def heads_of(t, B, H, dh):
    """(B * 81, H dh) -> (B, H, 81, dh)."""
    return t.reshape(B, S, H, dh).transpose(1, 2)


# (bf16, H, dh, B): B H = 9, 6, 3, 2, 5 (remainders 1, 2, 3 of the register form's four pairs per workgroup)
ATTN64_CASES = ((True, 3, 16, 3), (True, 3, 24, 2), (True, 3, 40, 1), (True, 2, 48, 1), (True, 1, 56, 2),
                (False, 3, 4, 2), (False, 2, 12, 1), (False, 1, 40, 2), (False, 2, 64, 1))
ATTN_BF16_FACTOR = 3.0                           # kernel error <= 3 x the error of the bf16-storage emulation (fp32 sums, fast exp on top)
ATTN_F32_TOL = 2e-5


@functools.lru_cache(maxsize=None)
def attn64_data(bf16, H, dh, B):
    g = torch.Generator().manual_seed(H * 100 + dh + B)
    dt = torch.bfloat16 if bf16 else torch.float32
    qkv = torch.randn(B * S, 3 * H * dh, generator=g).to(dt).float()
    dout = torch.randn(B * S, H * dh, generator=g).to(dt).float()
    return qkv, dout


def rel_l2(got, ref, dims):
    return ((got - ref).pow(2).sum(dims) / ref.pow(2).sum(dims)).sqrt()


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_vec_lanes(d, bf16, aligned=True):
    """ln_vec_lanes restated: lanes per row of the 16-byte kernels, 0 = one wave per row."""
    P = 8 if bf16 else 4
    if d % P or not aligned:
        return 0
    L = d // P
    return L if 1 <= L <= 64 and L & (L - 1) == 0 else 0


class LnCase(NamedTuple):
    bf16: bool
    M: int
    d: int
    off: int = 0                                 # every tensor starts this many elements past a 16-byte boundary
    far: bool = False                            # rows of mean 1000 and spread 1
    dres: bool = True

    @property
    def id(self):
        return f"{'bf16' if self.bf16 else 'f32'}-M{self.M}-d{self.d}" + ("-off" if self.off else "") + ("-far" if self.far else "") + ("" if self.dres else "-nodres")


def _ln_cases():
    """d: both ends of the 16-byte form (one lane per row; 64 lanes) and their neighbours that fall back (d / P = 3, 65), with
    M cycling through {1, 3, 127, 128, 129, 1000}; then every M at one d per type; offset, far-mean and no-residual cases."""
    Ms, out, i = (1, 3, 127, 128, 129, 1000), [], 0
    for bf16, ds in ((True, (8, 16, 24, 128, 256, 512, 520)), (False, (4, 12, 64, 256, 260))):
        for d in ds:
            out.append(LnCase(bf16, _cycle(Ms, i), d)); i += 1
        out += [LnCase(bf16, M, ds[3]) for M in Ms]
        out += [LnCase(bf16, 129, ds[3], off=1), LnCase(bf16, 127, ds[3], far=True), LnCase(bf16, 128, ds[0], dres=False),
                LnCase(bf16, 3, 24 if bf16 else 12, dres=False)]
    return tuple(dict.fromkeys(out))


LN_CASES = _ln_cases()
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_data(c: LnCase):
    """(x, gamma, beta, dy, dres) float32; x, dy, dres already rounded to the case's type."""
    g = torch.Generator().manual_seed(c.M * 131 + c.d + (1 if c.bf16 else 0))
    dt = torch.bfloat16 if c.bf16 else torch.float32
    x = torch.randn(c.M, c.d, generator=g)
    if c.far:                                    # mean 1000, spread about 1 on a grid fp32 sums exactly (bf16: its spacing at 1000 is 4), so the
        step = 4.0 if c.bf16 else 0.125          # case isolates the variance: E[x^2] - mean^2 in fp32 would lose it altogether
        x = 1000.0 + step * torch.randint(-1 if c.bf16 else -8, 2 if c.bf16 else 9, (c.M, c.d), generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(c.d, generator=g), 0.1 * torch.randn(c.d, generator=g)
    dy, dres = torch.randn(c.M, c.d, generator=g), torch.randn(c.M, c.d, generator=g)
    return x.to(dt).float(), gamma, beta, dy.to(dt).float(), dres.to(dt).float() if c.dres else None


def ln_ref(x, gamma, beta, dy, dres, mean=None, rstd=None, eps=LN_EPS):
    """fp64 from the kernel comments: y = (x - mean) rstd gamma + beta with the biased variance; from the mean and rstd HANDED
    to the backward (default: the forward's, unrounded) xhat = (x - mean) rstd, dx = rstd (g - mean(g) - xhat mean(g xhat))
    [+ dres], g = dy gamma; dgamma = sum dy xhat, dbeta = sum dy, with the sums of |terms| for their bounds."""
    x, gamma, beta, dy = x.double(), gamma.double(), beta.double(), dy.double()
    mean_f = x.mean(1, keepdim=True)
    rstd_f = ((x - mean_f).pow(2).mean(1, keepdim=True) + eps).rsqrt()
    y = (x - mean_f) * rstd_f * gamma + beta
    mean = mean_f if mean is None else mean.double()[:, None]
    rstd = rstd_f if rstd is None else rstd.double()[:, None]
    xh = (x - mean) * rstd
    gg = dy * gamma
    dx = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.double()
    return dict(y=y, mean=mean_f[:, 0], rstd=rstd_f[:, 0], dx=dx, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0),
                dgamma_abs=(dy * xh).abs().sum(0), dbeta_abs=dy.abs().sum(0), xabs=x.abs().mean(1))


def ln_row_bound(ref, bf16):
    """|got - ref| allowed on an output stored in the case's type: 2^-8 |ref| (bf16 rounding and one more ulp) + 1e-5 of the
    row's largest |ref|."""
    scale = ref.abs().amax(1, keepdim=True)
    return (2.0 ** -8 * ref.abs() if bf16 else 0.0) + 1e-5 * scale


# ------------------------------------------------------------------------------------------------ row kernels
COLSUM_CASES = tuple((M, N, ns) for ns, (M, N) in zip((1, 3, 8, 3, 8, 1, 3, 8), ((1, 1), (80, 255), (81, 256), (4097, 257), (80, 1),
                                                                                     (4097, 255), (1, 257), (81, 257))))
POS_GRAD_B = (1, 2, 63, 64, 65, 130)
TANH_NS = (1, 255, 256, 257, 1024 * 256 + 1)
# (M, N, ldi, ldo, bf16 input): the 16-byte bf16 transpose needs N % 8 == 0, ldi % 8 == 0, ldo % 8 == 0
TRANSPOSE_CASES = ((70, 72, 72, 96, True), (130, 8, 16, 160, True), (65, 200, 208, 96, True), (70, 45, 45, 96, True),
                   (70, 72, 76, 96, True), (70, 45, 48, 96, False), (33, 64, 64, 64, False))
CAST_CASES = ((70, 45, 45, 64, True), (70, 45, 48, 45, False), (1, 8, 8, 32, True), (300, 1000, 1000, 1024, False))


def transpose_vec(M, N, ldi, ldo, bf16):
    return bf16 and N % 8 == 0 and ldi % 8 == 0 and ldo % 8 == 0


def pos_grad_ranges(B):
    """Board ranges of pos_grad_kernel: min(B, 64) parts of ceil(B / parts) boards; trailing ones may be empty."""
    nz = min(B, 64)
    per = ceil_div(B, nz)
    return [(min(B, z * per), min(B, (z + 1) * per)) for z in range(nz)]


def colsum_ranges(M, nsplit):
    per = ceil_div(M, nsplit)
    return [(min(M, s * per), min(M, (s + 1) * per)) for s in range(nsplit)]


def ulp32(t):
    """One ulp of fp32 at t (fp64 tensor), taken as the relative unit 2^-23 |t|: between one and two spacings of fp32 at t.  A
    value that went through two fp32 roundings lies within it of the exact result ((1 + a)(1 + b) - 1 < 2^-23 for |a|, |b| <=
    2^-24 / (1 + 2^-24)), which is what tanh_bwd's statement is under contraction: fma(-y, y, 1), then the product."""
    return t.abs().clamp_min(2.0 ** -126) * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ guard-band cases
# Shared by tests/test_transformer_bounds_cpu.py and tests/test_hip_transformer_bounds.py.  The tile constants of
# csrc/transformer.hip beside BM / BN / K_TILE / TN_ROWS / SP above: kKsRows, kGM, kGN, the 128-column tiles of the TN kernel,
# the (board, head) pairs of a register-attention workgroup.
K256_ROWS, BIG_M, BIG_N, TN_COLS, ATTN_PAIRS = 128, 256, 256, 128, 4
GUARD_FLAT = 4096                                # elements on each side of a tensor a flat grid-stride kernel walks
# what one workgroup spans along the guarded (leading) dimension of its tensors, and the guard rows the tests put there
SPAN = {"tiled": max(BM, BN), "map": max(BM, BN), "k256": K256_ROWS, "big": max(BIG_M, BIG_N), "tn": max(TN_ROWS, TN_COLS),
        "attn": ATTN_PAIRS * SP}
GUARD_ROWS = {"tiled": 256, "map": 256, "k256": 256, "big": 512, "tn": 256, "attn": ATTN_PAIRS * SP}


def round8(n):
    return ceil_div(n, 8) * 8


def flat_rows(cols):
    """Guard rows of a (rows, cols) tensor that a flat kernel walks: at least GUARD_FLAT elements, a multiple of 8 rows."""
    return round8(ceil_div(GUARD_FLAT, cols))


def lse_guard(H):
    """Floats on each side of lse [B][H][81]: the four pairs of a workgroup, 96 padded squares each, for every head."""
    return ATTN_PAIRS * H * SP


def ln_block_rows(c):
    """The most rows one workgroup of a LayerNorm kernel owns: 4 waves x (64 / L) rows x 4 iterations in the 16-byte forward
    (4 rows in the wave-per-row one), ceil(M / parts) <= 128 in the backward."""
    L = ln_vec_lanes(c.d, c.bf16, not c.off)
    return max(128, 16 * (64 // L) if L else 4)


def ln_parts(M):
    """ka_tf_layernorm_parts restated."""
    return min(ceil_div(M, 128), 2048)


# ka_tf_gemm_nt on the tiled kernel: M in {1, 129}, N in {1, 130, 136}, K in {32, 96}; the scalar store (N or ldc no multiple
# of 4), the 8-byte one (bf16, multiples of 4), the 16-byte one (fp32, multiples of 4) and the LDS epilogue (bf16, multiples of
# 8, a full tile); the epilogue families none, bias + relu, bias + dropout + residual in fp32 and bf16; the masked entry once.
NT_BOUNDS_TILED = (NtCase("tiled", 1, 1, 32, "none", False),
                   NtCase("tiled", 129, 130, 96, "bias_relu", True, 8, 0, 1),
                   NtCase("tiled", 129, 136, 32, "bias_drop_res", True, 0, 8, 4),
                   NtCase("tiled", 1, 136, 96, "bias_drop_res", False, 8, 8, 0),
                   NtCase("tiled", 129, 136, 96, "bias_relu", False, 0, 0, 8),
                   NtCase("tiled", 1, 136, 32, "masked5", True, 8, 0, 0))
NT_BOUNDS_LDS = (NtCase("tiled", 129, 136, 96, "none", True, 0, 8, 0),)
NT_BOUNDS_SPLIT = (NT_SPLIT[0],)
# K = 256: the tail panel alone, one full panel and the tail, full panels only; N = 64 and 192; the residual and activation
# instantiations the C ABI reaches ((RES, ACT) = (1, 1) has no entry point)
NT_BOUNDS_K256 = tuple(NtCase("k256", M, N, 256, epi, True, la, lb, lc) for M, N, epi, la, lb, lc in
                       ((1, 64, "none", 0, 8, 0), (129, 192, "bias_drop_res", 8, 0, 8), (128, 64, "masked5", 0, 0, 8),
                        (129, 64, "res", 8, 8, 0), (1, 192, "masked0", 0, 8, 8), (128, 192, "bias_relu_drop", 8, 0, 0)))
NT_BOUNDS_BIG = (NT_BIG[2], NT_BIG[3])
NT_BOUNDS = NT_BOUNDS_TILED + NT_BOUNDS_LDS + NT_BOUNDS_SPLIT + NT_MAP + NT_BOUNDS_K256 + NT_BOUNDS_BIG
TN_BOUNDS = tuple(c for c in TN_CASES if (c.M, c.N, c.K) in ((1, 120, 264), (65, 264, 120), (4097, 136, 264)))
# register forms <1> (dh <= 16) and <2> with B H % 4 in {1, 2, 3}; the LDS forms at dh = 8 (by the switch), 40 and 64
HOT_BOUNDS_REG = (HotCase(1, 1, 8), HotCase(5, 1, 8), HotCase(3, 3, 16), HotCase(2, 5, 24), HotCase(1, 3, 32))
HOT_BOUNDS_LDS = (HotCase(5, 1, 8), HotCase(1, 3, 40), HotCase(1, 2, 64))
ATTN_BOUNDS_P = (0.0, 0.3, 0.5)                 # 0.5: the kept scale is exactly 2 and the one-hot oracle stays exact
LN_BOUNDS = ((LnCase(True, 1, 256), LnCase(True, 33, 256), LnCase(True, 1025, 8))
             + tuple(LnCase(bf, M, d) for bf in (False, True) for d, M in ((24, 1), (400, 5), (24, 129), (400, 1), (24, 5), (400, 129)))
             + (LnCase(True, 33, 256, off=1),))
W16_JOBS = ((8, 264), (139, 256), (70, 44))      # (N, K) of the three-job table of ka_tf_weights16_multi
DROP_BOUNDS_NS = (1, 5, 1025)
ROW_BOUNDS = ((1, 8), (3, 24))                   # (B, d) of add_pos, mean_pool, head_grad
POS_GRAD_BOUNDS_B = (1, 65)
TANH_BOUNDS_NS = (1, 257)

# every entry point with a pointer argument, by the group of cases that calls it (the coverage test of the CPU twin reads this)
BOUNDS_ENTRY_POINTS = {
    "ka_tf_gemm_nt": NT_BOUNDS, "ka_tf_gemm_nt_masked": tuple(c for c in NT_BOUNDS if c.masked),
    "ka_tf_gemm_tn": TN_BOUNDS, "ka_tf_gemm_tn_bias": TN_BOUNDS,
    "ka_tf_attention_fwd": HOT_BOUNDS_REG + HOT_BOUNDS_LDS, "ka_tf_attention_bwd": HOT_BOUNDS_REG + HOT_BOUNDS_LDS,
    "ka_tf_attention_bwd_o": HOT_BOUNDS_REG + HOT_BOUNDS_LDS,
    "ka_tf_layernorm_fwd": LN_BOUNDS, "ka_tf_layernorm_bwd": LN_BOUNDS, "ka_tf_layernorm_bwd_drop": LN_BOUNDS,
    "ka_tf_transpose_pad": TRANSPOSE_CASES, "ka_tf_cast_pad": CAST_CASES, "ka_tf_weights16_multi": W16_JOBS,
    "ka_tf_drop_apply": DROP_BOUNDS_NS, "ka_tf_add_pos": ROW_BOUNDS, "ka_tf_mean_pool": ROW_BOUNDS, "ka_tf_head_grad": ROW_BOUNDS,
    "ka_tf_colsum": COLSUM_CASES, "ka_tf_pos_grad": POS_GRAD_BOUNDS_B, "ka_tf_tanh": TANH_BOUNDS_NS, "ka_tf_tanh_bwd": TANH_BOUNDS_NS,
}
BOUNDS_NO_POINTERS_TO_GUARD = ("ka_tf_route_counts", "ka_tf_gemm_tn_slabs", "ka_tf_gemm_nt_slabs", "ka_tf_layernorm_parts")


def w16_ld(n):
    """Row length of the bf16 weight cache: the next multiple of 32 (hip/transformer.py)."""
    return ceil_div(n, 32) * 32


@functools.lru_cache(maxsize=None)
def w16_data(N, K):
    """(W fp32 (N, K), out (N, ldo) bf16, outT (K, ldt) bf16): the weight, its bf16 copy and the transposed copy, zero padded."""
    W = torch.randn(N, K, generator=torch.Generator().manual_seed(N * 1000 + K))
    out, outT = torch.zeros(N, w16_ld(K), dtype=torch.bfloat16), torch.zeros(K, w16_ld(N), dtype=torch.bfloat16)
    out[:, :K], outT[:, :N] = W.bfloat16(), W.t().bfloat16()
    return W, out, outT


# ------------------------------------------------------------------------------------------------ mutants of the references
def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def nt_mutant(**kw):
    return lambda c: same(nt_ref(c, *nt_data(c)[:6], **kw), nt_data(c).slabs)


def tn_mutant(**kw):
    return lambda c: same(tn_ref(c, tn_data(c).A, tn_data(c).B, **kw), tn_data(c)[2:])


def hot_mutant(which, **kw):
    """The mutant passes on a case if it does on both maps, with and without dropout (the GPU test runs all four); which:
    0 = out, 1 = dV."""
    def passes(case):
        return all(torch.equal(hot_ref(case, hot_data(case, many), SEED_BIG, p, **kw)[which], hot_ref(case, hot_data(case, many), SEED_BIG, p)[which])
                   for many in (False, True) for p in (0.0, 0.5))
    return passes


def hot_many_mutant(case):
    d = hot_data(case, True)
    return torch.equal(hot_ref(case, d, dv_last_only=True)[1], hot_ref(case, d)[1])


MUTANTS = {
    "last_k_tile_dropped": [(nt_mutant(drop_last_ktile=True), NT_CASES)],
    "mask_indexed_by_n": [(nt_mutant(mask_ld_n=True), tuple(c for c in NT_CASES if c.p and c.ldc_pad and c.M > 1))],
    "residual_before_dropout": [(nt_mutant(res_before_drop=True), tuple(c for c in NT_CASES if c.epi == "bias_drop_res"))],
    "activation_mask_ge": [(nt_mutant(act_ge=True), tuple(c for c in NT_CASES if c.masked and c.M * c.N >= 64))],
    "product_in_neighbouring_slab": [(nt_mutant(neighbour_slab=True), tuple(c for c in NT_CASES if len(c.ranges) > 1)),
                                     (tn_mutant(neighbour_slab=True), tuple(c for c in TN_CASES if c.slabs > 1))],
    "last_token_dropped": [(tn_mutant(drop_last_row=True), TN_CASES)],
    "key_column_80_dropped": [(hot_mutant(0, drop_key_80=True), HOT_CASES)],
    "next_heads_v": [(hot_mutant(0, next_head_v=True), tuple(c for c in HOT_CASES if c.H > 1))],
    "surplus_pair_not_repeated": [(hot_mutant(0, no_surplus_repeat=True), tuple(c for c in HOT_CASES if (c.B * c.H) % 4))],
    "dv_without_the_sum": [(hot_many_mutant, HOT_CASES)],
}
