"""Guard-band tests of the kernels of csrc/transformer.hip at their ragged shapes (the cases and guard sizes are proved on the
CPU by tests/test_transformer_bounds_cpu.py): every tensor argument is the middle of a larger allocation, with at least one whole
tile or workgroup span of the kernel before and after it (the rig of tests/test_hip_conv_bounds.py).  Guards of outputs and
workspaces hold a NaN bit pattern that must survive bit for bit; guards of inputs are zero in one run and NaN in a second, and the
outputs of the two runs must be finite and bit-identical; the valid region equals the oracle of tests/test_hip_transformer_exact.py
for the case, under that test's comparison; pad columns of C still hold the pattern; and the launch counters show the form the
case names.  Whatever a kernel could read or write past a tensor lies in memory the test owns: no test depends on a fault."""
import math

import pytest
import torch

from keisei_amd import _lib
import transformer_helpers as th
from test_hip_conv_bounds import PATTERN, bits, check_guarded
from test_hip_transformer_exact import assert_same, attention, delta, routes, st
from transformer_helpers import GUARD_FLAT, GUARD_ROWS, S, SEED_BIG, flat_rows, ints, round8

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
RUNS = 2                                         # check_guarded launches twice: zero and NaN input guards


def aligned(call, off=False):
    """The call, after a look at the pointers: 16-byte aligned (so the 16-byte paths are the ones that run), or every one off."""
    def checked(t):
        for n, v in t.items():
            assert (v.data_ptr() % 16 == 0) != bool(off), f"{n}: alignment"
        call(t)
    return checked


def tensor(t, rows, off=0):
    """An input / in-place entry of the rig: guard rows of t's leading dimension; with off, t flat and one element off."""
    if off:
        return t.flatten(), rows * (t.numel() // t.shape[0]), off
    return t, rows


def output(shape, dt, rows, off=0):
    if off:
        return (math.prod(shape),), dt, rows * (math.prod(shape) // shape[0]), off
    return tuple(shape), dt, rows


def pattern_kept(t):
    return bool((bits(t) == PATTERN[t.dtype][1]).all())


def moved_since(before):
    return {k: v for k, v in delta(before).items() if v}


# ------------------------------------------------------------------------------------------------ the rig, on the device
def test_rig_reports_a_row_too_many_on_the_device():
    """The rig sees what it is there for: a kernel told of one row more than its tensors hold (the extra row lies inside the
    guards, memory the test owns) is reported -- ka_tf_cast_pad writes that row, ka_tf_colsum only reads it."""
    M, N = 5, 24
    x = ints(torch.Generator().manual_seed(5), M, N)
    cast = lambda rows: aligned(lambda t: _lib.call("ka_tf_cast_pad", t["x"], t["out"], rows, N, N, N, _lib.DTYPE_F32, st()))
    spec = {"x": (x, flat_rows(N))}, {"out": ((M, N), BF16, flat_rows(N))}
    assert torch.equal(check_guarded(cast(M), *spec)["out"].cpu(), x.bfloat16())
    with pytest.raises(AssertionError, match="out: guard rows overwritten"):
        check_guarded(cast(M + 1), *spec)
    colsum = lambda rows: aligned(lambda t: _lib.call("ka_tf_colsum", t["a"], t["part"], t["out"], rows, N, 1, _lib.DTYPE_F32, st()))
    spec = {"a": (x, flat_rows(N))}, {"part": ((N,), F32, round8(N)), "out": ((N,), F32, GUARD_FLAT)}
    assert_same(check_guarded(colsum(M), *spec)["out"], x.double().sum(0), "colsum")
    with pytest.raises(AssertionError, match="non-finite"):
        check_guarded(colsum(M + 1), *spec)


# ------------------------------------------------------------------------------------------------ NT GEMM
def run_nt_guarded(case, expect=None):
    """ka_tf_gemm_nt / _masked with A, B, bias, residual, activation and C between guards (split K: eight whole slabs of M rows
    on each side of [ns][M][ldc]).  Returns the valid columns of C."""
    d = th.nt_data(case)
    cdt = BF16 if case.c_bf16 else F32
    ns, g = len(case.ranges), GUARD_ROWS[case.form]
    assert _lib.query("ka_tf_gemm_nt_slabs", case.K, case.nsplit) == ns
    ins = {"A": (d.A.to(BF16), g), "B": (d.B.to(BF16), g)}
    if d.bias is not None:
        ins["bias"] = (d.bias, GUARD_FLAT)
    if d.res is not None:
        ins["res"] = (d.res.to(cdt), g)
    if d.act is not None:
        ins["act"] = (d.act.to(BF16), g)

    def call(t):
        if case.masked:
            _lib.call("ka_tf_gemm_nt_masked", t["A"], t["B"], t["C"], t["act"], case.M, case.N, case.K, case.lda, case.ldb, case.ldc,
                      case.p, d.seed, st())
        else:
            _lib.call("ka_tf_gemm_nt", t["A"], t["B"], t["C"], t.get("bias"), t.get("res"), case.M, case.N, case.K, case.lda, case.ldb,
                      case.ldc, int(case.c_bf16), int("relu" in case.epi), case.nsplit, case.p, d.seed, st())

    before = routes()
    m = check_guarded(aligned(call), ins, {"C": ((ns * case.M, case.ldc), cdt, 8 * case.M if ns > 1 else g)},
                      valid={"C": lambda t: t[:, :case.N]})
    if expect is None:
        expect = {"k256": {"k256": 1}, "big": {"big": 1}, "map": {"map2d": 1}, "tiled": {}}[case.form]
        if case.form in ("map", "tiled") and th.nt_lds_epilogue(case):
            expect = dict(expect, lds_epi=1)
    assert moved_since(before) == {k: RUNS * v for k, v in expect.items()}, f"{case.id}: launch counts moved {moved_since(before)}"
    C = m["C"].view(ns, case.M, case.ldc)
    for s, slab in enumerate(d.slabs):
        assert_same(C[s, :, :case.N], slab, f"{case.id} slab {s} (K range {case.ranges[s]})")
    assert pattern_kept(C[:, :, case.N:]), f"{case.id}: pad columns of C written"
    return C[:, :, :case.N]


TILED = th.NT_BOUNDS_TILED + th.NT_BOUNDS_SPLIT


@pytest.mark.parametrize("case", TILED, ids=[c.id for c in TILED])
def test_gemm_nt_tiled_stays_inside_its_tensors(case):
    """gemm_nt_bf16_kernel at M = 1 and 129, N = 1, 130 and 136, K = 32 and 96: the scalar, 8-byte and 16-byte stores, the
    epilogue families in fp32 and bf16, ka_tf_gemm_nt_masked, and two split-K slabs between whole guard slabs."""
    run_nt_guarded(case)


@pytest.mark.parametrize("case", th.NT_BOUNDS_LDS, ids=[c.id for c in th.NT_BOUNDS_LDS])
def test_gemm_nt_lds_epilogue_stays_inside_its_tensors(ka_env, case):
    """One full tile through LDS beside ragged ones, with KA_TF_LDS_EPI on and off."""
    on = run_nt_guarded(case)
    ka_env.set("KA_TF_LDS_EPI", "0")
    off = run_nt_guarded(case, expect={"lds_epi_off": 1})
    assert torch.equal(on, off)


@pytest.mark.parametrize("case", th.NT_MAP, ids=[c.id for c in th.NT_MAP])
def test_gemm_nt_super_tile_map_stays_inside_its_tensors(case):
    """897 x 1025 x 64 on the super-tile map: the padding workgroups of the one-dimensional grid touch nothing."""
    run_nt_guarded(case)


@pytest.mark.parametrize("case", th.NT_BOUNDS_K256, ids=[c.id for c in th.NT_BOUNDS_K256])
def test_gemm_nt_k256_stays_inside_its_tensors(case):
    """gemm_nt_k256_kernel: the tail panel alone (M = 1), a full panel and the tail (129), full panels only (128), N = 64 and
    192, the plain, residual and activation instantiations."""
    run_nt_guarded(case)


@pytest.mark.parametrize("case", th.NT_BOUNDS_BIG, ids=[c.id for c in th.NT_BOUNDS_BIG])
def test_gemm_nt_big_tile_stays_inside_its_tensors(case):
    """gemm_nt_big_kernel at 1025 x 1027 x 1088: ragged 256 x 256 tiles along M and N, fp32 with bias and bf16 without."""
    run_nt_guarded(case)


# ------------------------------------------------------------------------------------------------ TN GEMM
@pytest.mark.parametrize("with_bias", [False, True], ids=["tn", "tn_bias"])
@pytest.mark.parametrize("case", th.TN_BOUNDS, ids=[c.id for c in th.TN_BOUNDS])
def test_gemm_tn_stays_inside_its_tensors(case, with_bias):
    """ka_tf_gemm_tn / _bias at one, two and four slabs: A, B, the slab set C and the column-sum slab set between guards."""
    d = th.tn_data(case)
    g = GUARD_ROWS["tn"]
    assert _lib.query("ka_tf_gemm_tn_slabs", case.M, case.nsplit) == case.slabs
    outs = {"C": ((case.slabs * case.N, case.ldc), F32, 8 * case.N)}
    if with_bias:
        outs["cs"] = ((case.slabs * case.N,), F32, GUARD_FLAT)

    def call(t):
        if with_bias:
            _lib.call("ka_tf_gemm_tn_bias", t["A"], t["B"], t["C"], t["cs"], case.M, case.N, case.K, case.lda, case.ldb, case.ldc,
                      case.nsplit, st())
        else:
            _lib.call("ka_tf_gemm_tn", t["A"], t["B"], t["C"], case.M, case.N, case.K, case.lda, case.ldb, case.ldc, case.nsplit, st())

    m = check_guarded(aligned(call), {"A": (d.A.to(BF16), g), "B": (d.B.to(BF16), g)}, outs, valid={"C": lambda t: t[:, :case.K]})
    C = m["C"].view(case.slabs, case.N, case.ldc)
    for z in range(case.slabs):
        assert_same(C[z, :, :case.K], d.slabs[z], f"{case.id} slab {z} (tokens {case.ranges[z]})")
    assert pattern_kept(C[:, :, case.K:]), f"{case.id}: pad columns of C written"
    if with_bias:
        assert_same(m["cs"].view(case.slabs, case.N), d.colsum, f"{case.id} column sums")


# ------------------------------------------------------------------------------------------------ attention
ATTN_PARAMS = ([(c, True, "reg") for c in th.HOT_BOUNDS_REG] + [(c, True, "one") for c in th.HOT_BOUNDS_REG]
               + [(c, bf, "lds") for c in th.HOT_BOUNDS_LDS for bf in (True, False)])


@pytest.mark.parametrize("p", th.ATTN_BOUNDS_P)
@pytest.mark.parametrize("case,bf16,form", ATTN_PARAMS, ids=[f"{c.id}-{'bf16' if bf else 'f32'}-{f}" for c, bf, f in ATTN_PARAMS])
def test_attention_stays_inside_its_tensors(ka_env, case, bf16, form, p):
    """ka_tf_attention_fwd, _bwd and _bwd_o with qkv, out, dout, lse and both dqkv between guards of four (board, head) pairs of
    96 padded squares: the register forms <1> and <2> with one, two and three pairs in the last workgroup (form "one":
    KA_TF_ATTN_ONE, the one-kernel backward behind _bwd_o too), the LDS forms at dh = 8 (bf16: by KA_TF_ATTN_LDS), 40 and 64
    (fp32 at 64: the lean backward).  The one-hot oracle of the exact test: at p = 0 and 0.5 out, lse, dQ = dK = 0 and dV bit for
    bit.  At p = 0.3 the kept probability 1 / 0.7 is no power of two and that oracle is not exact, so out must be zero exactly on the
    rows whose one probability the restated mask drops and nowhere else, and all four results must equal, bit for bit, those of
    the same calls on tensors allocated at exactly their size."""
    B, H, dh = case
    dt, d, g = (BF16 if bf16 else F32), H * dh, GUARD_ROWS["attn"]
    code = _lib.dtype_code(dt)
    if form == "lds" and th.attn_register_form(bf16, H, dh, B):
        ka_env.set("KA_TF_ATTN_LDS", "1")
    if form == "one":
        ka_env.set("KA_TF_ATTN_ONE", "1")
    outs = {"out": ((B * S, d), dt, g), "lse": ((B * H * S,), F32, th.lse_guard(H)), "g1": ((B * S, 3 * d), dt, g), "g2": ((B * S, 3 * d), dt, g)}

    def call(t):
        _lib.call("ka_tf_attention_fwd", t["qkv"], t["out"], t["lse"], B, H, dh, p, SEED_BIG, code, st())
        _lib.call("ka_tf_attention_bwd", t["qkv"], t["dout"], t["lse"], t["g1"], B, H, dh, p, SEED_BIG, code, st())
        _lib.call("ka_tf_attention_bwd_o", t["qkv"], t["out"], t["dout"], t["lse"], t["g2"], B, H, dh, p, SEED_BIG, code, st())

    for many in (False, True):
        data = th.hot_data(case, many)
        before = routes()
        m = check_guarded(aligned(call), {"qkv": (data.qkv.to(dt), g), "dout": (data.dout.to(dt), g)}, outs)
        moved = delta(before)
        assert (moved["attn_reg"], moved["attn_lds"]) == ((0, RUNS) if form == "lds" else (RUNS, 0)), moved
        what = f"{case.id} many={many} p={p}"
        lse = m["lse"].view(B, H, S)
        want_lse = torch.full((B, H, S), data.smax / math.sqrt(dh), dtype=torch.float64)
        assert torch.allclose(lse.double().cpu(), want_lse, rtol=1e-6, atol=0), what + " lse"
        if p in (0.0, 0.5):
            ref_out, ref_dv = th.hot_ref(case, data, SEED_BIG, p)
            assert_same(m["out"], ref_out, what + " out")
            for name in ("g1", "g2"):
                assert_same(m[name][:, :2 * d], torch.zeros(B * S, 2 * d, dtype=torch.float64), f"{what} {name} dQ | dK")
                assert_same(m[name][:, 2 * d:], ref_dv, f"{what} {name} dV")
            continue
        kept = (th.hot_keep(case, data, SEED_BIG, p) != 0).transpose(1, 2)[..., None].expand(B, S, H, dh)      # (B, 81, H, dh)
        assert torch.equal(m["out"].cpu().reshape(B, S, H, dh) != 0, kept), what + ": the rows dropout zeroes"
        plain = attention(data.qkv, data.dout, B, H, dh, p, SEED_BIG, dt)
        for name, got, want in zip(("out", "lse", "bwd", "bwd_o"), (m["out"], lse, m["g1"], m["g2"]), plain):
            assert torch.equal(bits(got), bits(want)), f"{what} {name}: differs from the call on exact-size tensors"


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("case", th.LN_BOUNDS, ids=[c.id for c in th.LN_BOUNDS])
def test_layernorm_stays_inside_its_tensors(case):
    """ka_tf_layernorm_fwd, _bwd and _bwd_drop: the 16-byte form with a block of 32 rows (d = 256) holding 1 and 33 rows and a
    block of 1024 rows (d = 8) at M = 1025, the wave-per-row form at d = 24 and 400, and every pointer one element off its
    alignment (wave form, the mask as a separate ka_tf_drop_apply pass).  x, dy, dres, gamma, beta, mean and rstd between input
    guards; y, mean, rstd, dx, dx_drop, dgamma, dbeta and the part workspace -- exactly ka_tf_layernorm_parts(M) * 2 * d floats,
    a whole copy of itself on each side -- between pattern guards.  The bounds are those of test_layernorm_against_fp64."""
    dt, code, M, d, off = (BF16 if case.bf16 else F32), int(case.bf16), case.M, case.d, case.off
    rows = th.ln_block_rows(case)
    x, gamma, beta, dy, dres = th.ln_data(case)
    fwd = th.ln_ref(x, gamma, beta, dy, dres)
    mean_in, rstd_in = fwd["mean"].float(), fwd["rstd"].float()
    ref = th.ln_ref(x, gamma, beta, dy, dres, mean_in, rstd_in)
    vec = lambda n: ((n,), F32, GUARD_FLAT, off)                 # an fp32 vector output
    act = lambda t: tensor(t.to(dt), rows, off)                  # a token tensor (M, d) in the case's type
    flat = lambda t: (t, GUARD_FLAT, off)                        # an fp32 vector input
    m = check_guarded(aligned(lambda t: _lib.call("ka_tf_layernorm_fwd", t["x"], t["gamma"], t["beta"], t["y"], t["mean"], t["rstd"], M, d,
                                                  th.LN_EPS, code, st()), off),
                      {"x": act(x), "gamma": flat(gamma), "beta": flat(beta)},
                      {"y": output((M, d), dt, rows, off), "mean": vec(M), "rstd": vec(M)})
    y = m["y"].view(M, d)
    err = (y.double().cpu() - ref["y"]).abs()
    assert bool((err <= th.ln_row_bound(ref["y"], case.bf16)).all()), f"y: worst {float((err / th.ln_row_bound(ref['y'], case.bf16)).max()):.2f} of the bound"
    assert bool(((m["mean"].double().cpu() - ref["mean"]).abs() <= 1e-6 * torch.maximum(ref["mean"].abs(), ref["xabs"])).all())
    assert torch.allclose(m["rstd"].double().cpu(), ref["rstd"], rtol=1e-6, atol=0)
    nparts = _lib.query("ka_tf_layernorm_parts", M)
    assert nparts == th.ln_parts(M)
    p, seed, results = 0.3, SEED_BIG, []
    ins = {"dy": act(dy), "x": act(x), "gamma": flat(gamma), "mean": flat(mean_in), "rstd": flat(rstd_in)}
    if dres is not None:
        ins["dres"] = act(dres)
    for fused in (False, True):
        outs = {"dx": output((M, d), dt, rows, off), "part": ((nparts * 2 * d,), F32, nparts * 2 * d, off), "dg": vec(d), "db": vec(d)}
        if fused:
            outs["dxd"] = output((M, d), dt, rows, off)
            call = lambda t: _lib.call("ka_tf_layernorm_bwd_drop", t["dy"], t["x"], t["gamma"], t["mean"], t["rstd"], t.get("dres"), t["dx"],
                                       t["dxd"], p, seed, t["part"], t["dg"], t["db"], M, d, code, st())
        else:
            call = lambda t: _lib.call("ka_tf_layernorm_bwd", t["dy"], t["x"], t["gamma"], t["mean"], t["rstd"], t.get("dres"), t["dx"],
                                       t["part"], t["dg"], t["db"], M, d, code, st())
        m = check_guarded(aligned(call, off), ins, outs)
        dx, dg, db = m["dx"].view(M, d), m["dg"], m["db"]
        results.append((dx.cpu(), dg.cpu(), db.cpu()))
        err = (dx.double().cpu() - ref["dx"]).abs()
        bound = th.ln_row_bound(ref["dx"], case.bf16)
        assert bool((err <= bound).all()), f"dx: worst {float((err / bound).max()):.2f} of the bound"
        for name, got in (("dgamma", dg), ("dbeta", db)):
            err, bound = (got.double().cpu() - ref[name]).abs(), M * 2.0 ** -23 * ref[name + "_abs"]
            assert bool((err <= bound).all()), f"{name}: worst {float((err / bound.clamp_min(1e-300)).max()):.3f} of the bound"
        if fused:
            keep = th.keep_mask(seed, M * d, p).reshape(M, d)
            scaled = (dx.float().cpu() * torch.tensor(th.inv_keep(p), dtype=F32)).to(dt)
            assert torch.equal(m["dxd"].view(M, d).cpu(), torch.where(keep, scaled, torch.zeros((), dtype=dt))), "dx_drop"
    assert all(torch.equal(a, b) for a, b in zip(*results)), "ka_tf_layernorm_bwd and _bwd_drop write the same dx, dgamma, dbeta"


# ------------------------------------------------------------------------------------------------ transposes, casts, weight cache
def tile_rows(ld):
    """Guard rows around a matrix the 64 x 64 (or 32 x 32) tile kernels walk: a whole tile, and GUARD_FLAT elements."""
    return max(flat_rows(ld), 64)


@pytest.mark.parametrize("M,N,ldi,ldo,bf16", th.TRANSPOSE_CASES)
def test_transpose_pad_stays_inside_its_tensors(M, N, ldi, ldo, bf16):
    dt = BF16 if bf16 else F32
    g = torch.Generator().manual_seed(M + N)
    x = th.padded(torch.randn(M, N, generator=g).to(dt).float(), ldi)
    m = check_guarded(aligned(lambda t: _lib.call("ka_tf_transpose_pad", t["x"], t["out"], M, N, ldi, ldo, _lib.dtype_code(dt), st())),
                      {"x": (x.to(dt), tile_rows(ldi))}, {"out": ((N, ldo), BF16, tile_rows(ldo))})
    want = torch.zeros(N, ldo, dtype=BF16)
    want[:, :M] = x[:, :N].t().bfloat16()
    assert torch.equal(m["out"].cpu(), want)


@pytest.mark.parametrize("M,N,ldi,ldo,bf16", th.CAST_CASES)
def test_cast_pad_stays_inside_its_tensors(M, N, ldi, ldo, bf16):
    dt = BF16 if bf16 else F32
    g = torch.Generator().manual_seed(M + N)
    x = th.padded(torch.randn(M, N, generator=g).to(dt).float(), ldi)
    m = check_guarded(aligned(lambda t: _lib.call("ka_tf_cast_pad", t["x"], t["out"], M, N, ldi, ldo, _lib.dtype_code(dt), st())),
                      {"x": (x.to(dt), flat_rows(ldi))}, {"out": ((M, ldo), BF16, flat_rows(ldo))})
    want = torch.zeros(M, ldo, dtype=BF16)
    want[:, :N] = x[:, :N].bfloat16()
    assert torch.equal(m["out"].cpu(), want)


def test_weights16_multi_stays_inside_its_tensors():
    """Three jobs in one launch, (N, K) = (8, 264), (139, 256), (70, 44): every W, out and outT its own guarded tensor, the job
    table between eight rows of zeros (jobs of no rows and no columns, should the search step outside)."""
    jobs = th.W16_JOBS
    data = [th.w16_data(N, K) for N, K in jobs]
    ins = {f"W{i}": (W, tile_rows(W.shape[1])) for i, (W, _, _) in enumerate(data)}
    outs = {}
    for i, (_, o, oT) in enumerate(data):
        outs[f"o{i}"] = (tuple(o.shape), BF16, tile_rows(o.shape[1]))
        outs[f"t{i}"] = (tuple(oT.shape), BF16, tile_rows(oT.shape[1]))

    def call(t):
        rows, first = [], 0
        for i, (N, K) in enumerate(jobs):
            o, oT = t[f"o{i}"], t[f"t{i}"]
            rows.append([t[f"W{i}"].data_ptr(), o.data_ptr(), oT.data_ptr(), N, K, o.shape[1], oT.shape[1], first])
            first += th.ceil_div(oT.shape[1], 64) * th.ceil_div(o.shape[1], 64)
        table = torch.zeros(8 + len(jobs) + 8, 8, dtype=torch.int64)
        table[8:8 + len(jobs)] = torch.tensor(rows, dtype=torch.int64)
        table = table.to(DEV)
        _lib.call("ka_tf_weights16_multi", table[8:8 + len(jobs)], len(jobs), first, st())
        torch.cuda.synchronize()

    m = check_guarded(aligned(call), ins, outs)
    for i, (_, o, oT) in enumerate(data):
        assert torch.equal(m[f"o{i}"].cpu(), o), f"job {i} {jobs[i]}: out"
        assert torch.equal(m[f"t{i}"].cpu(), oT), f"job {i} {jobs[i]}: outT"


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off"])
@pytest.mark.parametrize("n", th.DROP_BOUNDS_NS)
def test_drop_apply_stays_inside_its_tensors(n, off, dt):
    """out = 2 g keep [act > 0] + res at p = 0.5 on integers, one element, a scalar tail and more than one block, 16-byte
    aligned and every pointer one element off (all scalar)."""
    code = _lib.dtype_code(dt)
    g = torch.Generator().manual_seed(11 + n)
    x, act, res = ints(g, n), th.zeros_and_signs(g, n), ints(g, n)
    keep = th.keep_mask(SEED_BIG, n, 0.5)
    for use_act, use_res in ((True, False), (False, True), (True, True)):
        ins = {"x": (x.to(dt), GUARD_FLAT, off)}
        if use_act:
            ins["act"] = (act.to(dt), GUARD_FLAT, off)
        if use_res:
            ins["res"] = (res.to(dt), GUARD_FLAT, off)
        m = check_guarded(aligned(lambda t: _lib.call("ka_tf_drop_apply", t["x"], t.get("act"), t.get("res"), t["out"], n, 0.5, SEED_BIG,
                                                      code, st()), off), ins, {"out": ((n,), dt, GUARD_FLAT, off)})
        want = 2.0 * x.double() * keep * ((act > 0) if use_act else 1) + (res.double() if use_res else 0)
        assert_same(m["out"], want, f"n={n} off={off} act={use_act} res={use_res}")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,d", th.ROW_BOUNDS)
def test_add_pos_mean_pool_head_grad_stay_inside_their_tensors(dt, B, d):
    code, M, rows = _lib.dtype_code(dt), B * S, flat_rows(d)
    g = torch.Generator().manual_seed(B + d)
    x, rowe, cole = ints(g, M, d), ints(g, 9, d), ints(g, 9, d)
    m = check_guarded(aligned(lambda t: _lib.call("ka_tf_add_pos", t["x"], t["rowe"], t["cole"], B, d, code, st())),
                      {"rowe": (rowe, rows), "cole": (cole, rows)}, {}, inout={"x": (x.to(dt), rows)})
    s = torch.arange(M) % S
    assert_same(m["x"], x.double() + rowe.double()[s // 9] + cole.double()[s % 9], "add_pos")
    x81 = 81.0 * ints(g, M, d)
    m = check_guarded(aligned(lambda t: _lib.call("ka_tf_mean_pool", t["x"], t["pooled"], B, d, code, st())),
                      {"x": (x81.to(dt), rows)}, {"pooled": ((B, d), F32, rows)})
    assert_same(m["pooled"], x81.double().reshape(B, S, d).sum(1) / 81.0, "mean_pool")
    dpooled, dflat = 81.0 * ints(g, B, d), ints(g, M, d)
    for use_p, use_f in ((True, True), (True, False), (False, True)):
        ins = {}
        if use_p:
            ins["dpooled"] = (dpooled, rows)
        if use_f:
            ins["dflat"] = (dflat.to(dt), rows)
        m = check_guarded(aligned(lambda t: _lib.call("ka_tf_head_grad", t.get("dpooled"), t.get("dflat"), t["dx"], B, d, code, st())),
                          ins, {"dx": ((M, d), dt, rows)})
        want = (dpooled.double() / 81.0).repeat_interleave(S, 0) * use_p + dflat.double() * use_f
        assert_same(m["dx"], want, f"head_grad pooled={use_p} flat={use_f}")


@pytest.mark.parametrize("M,N,nsplit", th.COLSUM_CASES)
def test_colsum_stays_inside_its_tensors(M, N, nsplit):
    """part is exactly nsplit * N floats, with at least a whole copy of itself on each side."""
    g = torch.Generator().manual_seed(M + N)
    a = ints(g, M, N)
    for dt in (F32, BF16):
        m = check_guarded(aligned(lambda t: _lib.call("ka_tf_colsum", t["a"], t["part"], t["out"], M, N, nsplit, _lib.dtype_code(dt), st())),
                          {"a": (a.to(dt), flat_rows(N))}, {"part": ((nsplit * N,), F32, round8(nsplit * N)), "out": ((N,), F32, GUARD_FLAT)})
        assert_same(m["out"], a.double().sum(0), "colsum")
        assert_same(m["part"].view(nsplit, N), torch.stack([a.double()[b:e].sum(0) for b, e in th.colsum_ranges(M, nsplit)]), "colsum parts")


@pytest.mark.parametrize("B", th.POS_GRAD_BOUNDS_B)
def test_pos_grad_stays_inside_its_tensors(B):
    """scratch is exactly 65 * 81 * d floats (the result and up to 64 parts), a whole copy of itself on each side; at B = 1 only
    two of its 65 rows are written, so it is held to its guards alone."""
    d = 24
    g = torch.Generator().manual_seed(B)
    dx = ints(g, B * S, d)
    tot = dx.double().reshape(B, 9, 9, d).sum(0)
    n = 65 * 81 * d
    for dt in (F32, BF16):
        m = check_guarded(aligned(lambda t: _lib.call("ka_tf_pos_grad", t["dx"], t["scratch"], t["drow"], t["dcol"], B, d, _lib.dtype_code(dt), st())),
                          {"dx": (dx.to(dt), max(flat_rows(d), round8(S)))},
                          {"scratch": ((n,), F32, n), "drow": ((9, d), F32, flat_rows(d)), "dcol": ((9, d), F32, flat_rows(d))},
                          finite={"drow", "dcol"})
        assert_same(m["drow"], tot.sum(1), f"drow B={B}")
        assert_same(m["dcol"], tot.sum(0), f"dcol B={B}")


@pytest.mark.parametrize("n", th.TANH_BOUNDS_NS)
def test_tanh_and_its_backward_stay_inside_their_tensors(n):
    """tanh in place to 2 ulp of fp32, tanh_bwd to 1: the bounds of test_tanh_and_its_backward."""
    g = torch.Generator().manual_seed(n)
    x, dy = 3 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    m = check_guarded(aligned(lambda t: _lib.call("ka_tf_tanh", t["v"], n, st())), {}, {}, inout={"v": (x, GUARD_FLAT)})
    ref = torch.tanh(x.double())
    assert float(((m["v"].double().cpu() - ref).abs() / th.ulp32(ref)).max()) <= 2
    y = m["v"].cpu()
    m = check_guarded(aligned(lambda t: _lib.call("ka_tf_tanh_bwd", t["dy"], t["y"], t["dx"], n, st())),
                      {"dy": (dy, GUARD_FLAT), "y": (y, GUARD_FLAT)}, {"dx": ((n,), F32, GUARD_FLAT)})
    ref = dy.double() * (1 - y.double() ** 2)
    assert float(((m["dx"].double().cpu() - ref).abs() / th.ulp32(ref)).max()) <= 1
