"""The kernels of csrc/transformer.hip held to the oracles of tests/transformer_helpers.py (proved on the CPU by
tests/test_transformer_exact_cpu.py).

Exact, torch.equal against fp64: the dropout mask against its integer restatement; the NT GEMM on every form (tiled with every
store path and epilogue, split-K slab by slab, the super-tile map, the K = 256 and the 256 x 256 tile forms -- each case asserts
its route from ka_tf_route_counts) and the TN GEMM slab by slab with its column sums, on integer operands between NaN pad
columns; attention through a one-hot softmax (out is a row of V, dV a sum of rows of dout, dQ = dK = 0) on the LDS and the
register kernels, both backward entry points, with and without dropout; the row kernels on integers.
Bounded, derived from the formats: LayerNorm forward / backward / backward with the dropped second output against fp64;
attention on random operands against fp64 (fp32: 2e-5; bf16: at most ATTN_BF16_FACTOR times the error of the oracle's own
bf16-storage emulation); tanh to 2 ulp, its backward to 1.
Every output and every pad column is NaN before the launch: an unwritten or overwritten element shows."""
import math

import pytest
import torch

from keisei_amd import _lib
import transformer_helpers as th
from transformer_helpers import (ATTN64_CASES, ATTN_BF16_FACTOR, ATTN_F32_TOL, CAST_CASES, COLSUM_CASES, DROP_NS, DROP_PS, HOT_CASES,
                                 LN_CASES, NAN, NT_BIG, NT_K256, NT_LDS, NT_MAP, NT_SPLIT, NT_TILED, POS_GRAD_B, S, SEED_BIG,
                                 SEED_SMALL, TANH_NS, TN_CASES, TRANSPOSE_CASES, ints)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
ROUTE_NAMES = ("k256", "big", "map2d", "map2d_off", "lds_epi", "lds_epi_off", "attn_reg", "attn_lds")


def st():
    return _lib.stream_ptr()


def sync():
    torch.cuda.synchronize()


def routes():
    out = torch.zeros(len(ROUTE_NAMES), dtype=torch.int64)
    _lib.call("ka_tf_route_counts", out.data_ptr(), len(ROUTE_NAMES))
    return dict(zip(ROUTE_NAMES, out.tolist()))


def delta(before):
    return {k: v - before[k] for k, v in routes().items()}


def place(t, dtype=F32, off=0):
    """t on the device in dtype, contiguous, starting `off` elements past a 16-byte aligned address."""
    if t is None:
        return None
    flat = torch.zeros(t.numel() + off, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    flat[off:].copy_(t.flatten().to(dtype))
    return flat[off:].view(t.shape)


def nans(*shape, dtype=F32, off=0):
    return torch.full((math.prod(shape) + off,), NAN, dtype=dtype, device=DEV)[off:].view(shape)


def assert_same(got, expected, what):
    """torch.equal of a device result with an fp64 reference rounded once to the result's dtype."""
    got = got.cpu()
    expected = expected.float().to(got.dtype) if expected.dtype == torch.float64 else expected
    if not torch.equal(got, expected):
        diff = (got.double() - expected.double()).abs().nan_to_num(nan=float("inf")).flatten()
        i = int(diff.argmax())
        pytest.fail(f"{what}: {int((diff != 0).sum())} of {diff.numel()} entries differ, worst at flat index {i} of shape "
                    f"{tuple(got.shape)}: got {float(got.flatten()[i])}, expected {float(expected.flatten()[i])}")


# ------------------------------------------------------------------------------------------------ the dropout mask
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", DROP_PS)
def test_drop_apply_on_ones_is_the_restated_mask(dt, p):
    """ka_tf_drop_apply(ones) == keep_mask / (1 - p) rounded to the type: every n (the scalar tail n % 4 / n % 8, one element,
    more than one block), a base one element off its alignment (vec == 0: all scalar), seeds below and above 2^32."""
    code = _lib.dtype_code(dt)
    kept = torch.tensor(th.inv_keep(p), dtype=F32).to(dt)
    for n in DROP_NS:
        for off in (0, 1):
            for seed in (SEED_SMALL, SEED_BIG):
                x, out = place(torch.ones(n), dt, off), nans(n, dtype=dt, off=off)
                assert (x.data_ptr() % 16 != 0) == bool(off) and (out.data_ptr() % 16 != 0) == bool(off)
                _lib.call("ka_tf_drop_apply", x, None, None, out, n, p, seed, code, st())
                sync()
                want = torch.where(th.keep_mask(seed, n, p), kept, torch.zeros((), dtype=dt))
                assert torch.equal(out.cpu(), want), (n, off, seed)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_drop_apply_activation_and_residual_forms(dt):
    """p = 0.5 on integers: out = 2 g keep [act > 0] + res exactly; act holds +0.0 and -0.0, which both drop."""
    code = _lib.dtype_code(dt)
    g = torch.Generator().manual_seed(11)
    for n in (5, 1025, 81 * 24 + 1):
        for off in (0, 1):
            x, act, res = ints(g, n), th.zeros_and_signs(g, n), ints(g, n)
            assert n < 64 or (bool(((act == 0) & torch.signbit(act)).any()) and bool(((act == 0) & ~torch.signbit(act)).any()))
            keep = th.keep_mask(SEED_BIG, n, 0.5)
            for use_act, use_res in ((True, False), (False, True), (True, True)):
                out = nans(n, dtype=dt, off=off)
                _lib.call("ka_tf_drop_apply", place(x, dt, off), place(act, dt, off) if use_act else None,
                          place(res, dt, off) if use_res else None, out, n, 0.5, SEED_BIG, code, st())
                sync()
                want = 2.0 * x.double() * keep * ((act > 0) if use_act else 1) + (res.double() if use_res else 0)
                assert_same(out, want, f"n={n} off={off} act={use_act} res={use_res}")


# ------------------------------------------------------------------------------------------------ NT GEMM
def run_nt(case, expect=None):
    """One call on NaN-filled slabs of M x ldc: every slab equal to its reference, pad columns still NaN, and the launch counts
    show the form the case names (expect: the counters that must have moved instead).  Returns the slabs on the device."""
    d = th.nt_data(case)
    cdt = BF16 if case.c_bf16 else F32
    ns = len(case.ranges)
    assert _lib.query("ka_tf_gemm_nt_slabs", case.K, case.nsplit) == ns
    A, B = place(d.A, BF16), place(d.B, BF16)
    C = nans(ns, case.M, case.ldc, dtype=cdt)
    before = routes()
    if case.masked:
        _lib.call("ka_tf_gemm_nt_masked", A, B, C, place(d.act, BF16), case.M, case.N, case.K, case.lda, case.ldb, case.ldc, case.p,
                  d.seed, st())
    else:
        _lib.call("ka_tf_gemm_nt", A, B, C, place(d.bias), place(d.res, cdt), case.M, case.N, case.K, case.lda, case.ldb, case.ldc,
                  int(case.c_bf16), int("relu" in case.epi), case.nsplit, case.p, d.seed, st())
    sync()
    moved = {k: v for k, v in delta(before).items() if v and not k.startswith("attn")}
    if expect is None:
        expect = {"k256": {"k256": 1}, "big": {"big": 1}, "map": {"map2d": 1}, "tiled": {}}[case.form]
        if case.form in ("map", "tiled") and th.nt_lds_epilogue(case):
            expect = dict(expect, lds_epi=1)
    assert moved == expect, f"{case.id}: launch counts moved {moved}, expected {expect}"
    for s, slab in enumerate(d.slabs):
        assert_same(C[s, :, :case.N], slab, f"{case.id} slab {s} (K range {case.ranges[s]})")
    assert bool(torch.isnan(C[:, :, case.N:]).all()), f"{case.id}: pad columns of C written"
    return C[:, :, :case.N]


@pytest.mark.parametrize("case", NT_TILED + NT_SPLIT, ids=[c.id for c in NT_TILED + NT_SPLIT])
def test_gemm_nt_tiled_exact(case):
    """gemm_nt_bf16_kernel: the scalar, 8 / 16-byte and LDS store paths and their boundaries, a trailing half k-tile, operand
    rows wider than K, C rows wider than N, every epilogue in fp32 and bf16 (dropout index row * ldc + col: each dropout case
    at two ldc), and split K with every slab against its own K range."""
    run_nt(case)


@pytest.mark.parametrize("case", NT_LDS, ids=[c.id for c in NT_LDS])
def test_gemm_nt_lds_epilogue_on_and_off(ka_env, case):
    """Full and ragged tiles in one launch: the full ones leave through LDS, with KA_TF_LDS_EPI=0 through the registers."""
    on = run_nt(case)
    ka_env.set("KA_TF_LDS_EPI", "0")
    off = run_nt(case, expect={"lds_epi_off": 1})
    assert torch.equal(on, off)


@pytest.mark.parametrize("case", NT_MAP, ids=[c.id for c in NT_MAP])
def test_gemm_nt_super_tile_map_exact(ka_env, case):
    """9 x 8 tiles: the one-dimensional grid walked as 8 x 8 super-tiles per XCD (padding workgroups exit), and KA_TF_MAP2D=0."""
    mapped = run_nt(case)
    ka_env.set("KA_TF_MAP2D", "0")
    plain = run_nt(case, expect={"map2d_off": 1})
    assert torch.equal(mapped, plain)


@pytest.mark.parametrize("case", NT_K256, ids=[c.id for c in NT_K256])
def test_gemm_nt_k256_exact(ka_env, case):
    """gemm_nt_k256_kernel: full panels only, the tail only, both; its residual and activation instantiations; ldc = N + 8 and
    operand rows of 264; N = 272 (no multiple of 64) stays on the tiled kernel.  KA_TF_K256=0 gives the same bits."""
    k256 = run_nt(case)
    if case.form == "k256":
        ka_env.set("KA_TF_K256", "0")
        c = case._replace(form="tiled")
        assert torch.equal(k256, run_nt(c))


@pytest.mark.parametrize("case", NT_BIG, ids=[c.id for c in NT_BIG])
def test_gemm_nt_big_tile_exact(case):
    """gemm_nt_big_kernel: one whole super-tile, a partial one with N % 4 != 0 (scalar stores), a second super column; fp32 with
    bias and bf16 with ldc rounded up to 8; K = 1056 is no multiple of 64 and stays on the tiled kernel."""
    run_nt(case)


# ------------------------------------------------------------------------------------------------ TN GEMM
@pytest.mark.parametrize("case", TN_CASES, ids=[c.id for c in TN_CASES])
def test_gemm_tn_exact(case):
    """Each slab and each column-sum slab against its own token range: slab counts on both sides of the kernel's groups of 8,
    one to three tiles along N and K, NaN pad columns in both operands, 16-byte and scalar stores of C."""
    d = th.tn_data(case)
    assert _lib.query("ka_tf_gemm_tn_slabs", case.M, case.nsplit) == case.slabs
    A, B = place(d.A, BF16), place(d.B, BF16)
    for with_bias in (False, True):
        C, cs = nans(case.slabs, case.N, case.ldc), nans(case.slabs, case.N)
        if with_bias:
            _lib.call("ka_tf_gemm_tn_bias", A, B, C, cs, case.M, case.N, case.K, case.lda, case.ldb, case.ldc, case.nsplit, st())
        else:
            _lib.call("ka_tf_gemm_tn", A, B, C, case.M, case.N, case.K, case.lda, case.ldb, case.ldc, case.nsplit, st())
        sync()
        for z in range(case.slabs):
            assert_same(C[z, :, :case.K], d.slabs[z], f"{case.id} slab {z} (tokens {case.ranges[z]})")
        assert bool(torch.isnan(C[:, :, case.K:]).all()), f"{case.id}: pad columns of C written"
        if with_bias:
            assert_same(cs, d.colsum, f"{case.id} column sums")
        else:
            assert bool(torch.isnan(cs).all())


# ------------------------------------------------------------------------------------------------ attention, one-hot
def attention(qkv, dout, B, H, dh, p, seed, dt):
    """(out, lse, dqkv of ka_tf_attention_bwd, dqkv of ka_tf_attention_bwd_o fed the forward's output) on the device."""
    code, d = _lib.dtype_code(dt), H * dh
    q, do = place(qkv, dt), place(dout, dt)
    out, lse = nans(B * S, d, dtype=dt), nans(B, H, S)
    _lib.call("ka_tf_attention_fwd", q, out, lse, B, H, dh, p, seed, code, st())
    g1, g2 = nans(B * S, 3 * d, dtype=dt), nans(B * S, 3 * d, dtype=dt)
    _lib.call("ka_tf_attention_bwd", q, do, lse, g1, B, H, dh, p, seed, code, st())
    _lib.call("ka_tf_attention_bwd_o", q, out, do, lse, g2, B, H, dh, p, seed, code, st())
    sync()
    return out, lse, g1, g2


def attn_forms(bf16, H, dh, B):
    return ("reg", "lds") if th.attn_register_form(bf16, H, dh, B) else ("lds",)


HOT_PARAMS = [(c, bf, form) for c in HOT_CASES for bf in (False, True) for form in attn_forms(bf, c.H, c.dh, c.B)]


@pytest.mark.parametrize("case,bf16,form", HOT_PARAMS, ids=[f"{c.id}-{'bf16' if bf else 'f32'}-{f}" for c, bf, f in HOT_PARAMS])
def test_attention_one_hot_exact(ka_env, case, bf16, form):
    """Every query is one key (a sign vector of magnitude c) under the weights of HotCase.weights: the softmax is exactly one-hot, so out[b, s, h] = V[b, phi(s), h]
    (times 2 or 0 under dropout at p = 0.5, by the mask at ((b H + h) 96 + s) 96 + phi(s)), lse = the selected score, dQ = dK = 0
    and dV[t] = the sum of (the kept, doubled) dout[s] over phi(s) = t -- bit for bit, for a permutation and a many-to-one phi
    drawn per (board, head).  fp32 at dh = 48, 56, 64 runs the backward form without transposed LDS copies (the full form does
    not fit the LDS there and the launch failed before that form existed).  A wrong head offset, board stride, tile column or surplus wave cannot pass."""
    B, H, dh = case
    dt, d = (BF16 if bf16 else F32), H * dh
    if bf16 and form == "lds":
        ka_env.set("KA_TF_ATTN_LDS", "1")
    for many in (False, True):
        data = th.hot_data(case, many)
        for p in (0.0, 0.5):
            before = routes()
            out, lse, g1, g2 = attention(data.qkv, data.dout, B, H, dh, p, SEED_BIG, dt)
            moved = delta(before)
            assert (moved["attn_reg"], moved["attn_lds"]) == ((1, 0) if form == "reg" else (0, 1)), moved
            ref_out, ref_dv = th.hot_ref(case, data, SEED_BIG, p)
            what = f"{case.id} many={many} p={p}"
            assert_same(out, ref_out, what + " out")
            want_lse = torch.full((B, H, S), data.smax / math.sqrt(dh), dtype=torch.float64)
            assert torch.allclose(lse.double().cpu(), want_lse, rtol=1e-6, atol=0), what + " lse"
            for name, g in (("bwd", g1), ("bwd_o", g2)):
                assert_same(g[:, :2 * d], torch.zeros(B * S, 2 * d, dtype=torch.float64), f"{what} {name} dQ | dK")
                assert_same(g[:, 2 * d:], ref_dv, f"{what} {name} dV")


# ------------------------------------------------------------------------------------------------ attention, fp64 oracle
ATTN64_PARAMS = [(bf, H, dh, B, form) for bf, H, dh, B in ATTN64_CASES for form in attn_forms(bf, H, dh, B)]


@pytest.mark.parametrize("bf16,H,dh,B,form", ATTN64_PARAMS, ids=[f"{'bf16' if bf else 'f32'}-H{H}-dh{dh}-B{B}-{f}" for bf, H, dh, B, f in ATTN64_PARAMS])
def test_attention_against_fp64(ka_env, bf16, H, dh, B, form):
    """Random operands at the head shapes no other kernel-level test runs.  fp32: out and lse to 2e-5, dQ, dK, dV each to 2e-5
    relative L2.  bf16: the relative L2 error of out per (board, head) and of dQ, dK, dV may be at most ATTN_BF16_FACTOR times the
    error the fp64 oracle makes itself when it stores bf16 where the kernels do (P before P V, dS and P before their products,
    outputs rounded once; for ka_tf_attention_bwd_o with D = rowsum(dO O) from the rounded output).
    Measured on MI355X (kernel error / emulation error): see DESIGN.md section 2."""
    dt, d = (BF16 if bf16 else F32), H * dh
    if bf16 and form == "lds":
        ka_env.set("KA_TF_ATTN_LDS", "1")
    qkv, dout = th.attn64_data(bf16, H, dh, B)
    before = routes()
    out, lse, g1, g2 = attention(qkv, dout, B, H, dh, 0.0, 0, dt)
    moved = delta(before)
    assert (moved["attn_reg"], moved["attn_lds"]) == ((1, 0) if form == "reg" else (0, 1)), moved
    ref = th.attn_ref64(qkv, dout, B, H, dh)
    out_h, lse = th.heads_of(out.double().cpu(), B, H, dh), lse.double().cpu()
    assert torch.allclose(lse, ref[1], rtol=1e-5, atol=ATTN_F32_TOL), float((lse - ref[1]).abs().max())
    grads = {n: [th.heads_of(g.double().cpu()[:, i * d:(i + 1) * d], B, H, dh) for i in range(3)] for n, g in (("bwd", g1), ("bwd_o", g2))}
    if not bf16:
        assert torch.allclose(out_h, ref[0], rtol=ATTN_F32_TOL, atol=ATTN_F32_TOL), float((out_h - ref[0]).abs().max())
        for n, gs in grads.items():
            for i, what in enumerate(("dQ", "dK", "dV")):
                e = float(th.rel_l2(gs[i], ref[2 + i], (0, 1, 2, 3)))
                print(f"{n} {what}: relative L2 {e:.2e}")
                assert e < ATTN_F32_TOL, (n, what, e)
        return
    worst = {}
    for n, gs in grads.items():
        emu = th.attn_ref64(qkv, dout, B, H, dh, emulate=True, d_from_out=(n == "bwd_o"))
        ratio = th.rel_l2(out_h, ref[0], (2, 3)) / th.rel_l2(emu[0], ref[0], (2, 3))
        worst[f"{n} out"] = float(ratio.max())
        for i, what in enumerate(("dQ", "dK", "dV")):
            worst[f"{n} {what}"] = float(th.rel_l2(gs[i], ref[2 + i], (0, 1, 2, 3)) / th.rel_l2(emu[2 + i], ref[2 + i], (0, 1, 2, 3)))
    print(f"bf16 H={H} dh={dh} B={B} {form}: kernel error / emulation error " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v <= ATTN_BF16_FACTOR for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("case", LN_CASES, ids=[c.id for c in LN_CASES])
def test_layernorm_against_fp64(case):
    """Forward, backward and the backward with the dropped second output.  Outputs stored in the type: |got - ref| <= 2^-8 |ref|
    (bf16 only) + 1e-5 of the row's largest |ref|; mean to 1e-6 of max(|mean|, the row's mean |x|) (relative to a mean near zero
    no fp32 sum can hold), rstd to 1e-6 relative; dgamma / dbeta, fp32 sums of M terms read from the same inputs as the reference
    (the backward's mean and rstd are the reference's, rounded to fp32): M 2^-23 sum |terms| per column; dx_drop exactly 0 where
    keep_mask says so, else the stored dx times fp32 1 / (1 - p), rounded to the type.
    Measured on MI355X, worst |error| / bound of dgamma: 0.49 at M = 1, 0.31 at M = 3, below 0.01 from M = 127 on.  (With
    the term dy * xhat taken from the fp32 xhat -- three roundings of its own -- the M = 1 cases measured up to 1.19; the
    kernels now form each term in double and round it once.)"""
    dt, code, M, d = (BF16 if case.bf16 else F32), int(case.bf16), case.M, case.d
    x, gamma, beta, dy, dres = th.ln_data(case)
    fwd = th.ln_ref(x, gamma, beta, dy, dres)
    mean_in, rstd_in = fwd["mean"].float(), fwd["rstd"].float()
    ref = th.ln_ref(x, gamma, beta, dy, dres, mean_in, rstd_in)
    xd, dyd, drd = place(x, dt, case.off), place(dy, dt, case.off), place(dres, dt, case.off)
    gd, bd = place(gamma), place(beta)
    y, mu, rs = nans(M, d, dtype=dt, off=case.off), nans(M), nans(M)
    _lib.call("ka_tf_layernorm_fwd", xd, gd, bd, y, mu, rs, M, d, th.LN_EPS, code, st())
    sync()
    err = (y.double().cpu() - ref["y"]).abs()
    assert bool((err <= th.ln_row_bound(ref["y"], case.bf16)).all()), f"y: worst {float((err / th.ln_row_bound(ref['y'], case.bf16)).max()):.2f} of the bound"
    assert bool(((mu.double().cpu() - ref["mean"]).abs() <= 1e-6 * torch.maximum(ref["mean"].abs(), ref["xabs"])).all())
    assert torch.allclose(rs.double().cpu(), ref["rstd"], rtol=1e-6, atol=0)
    nparts = _lib.query("ka_tf_layernorm_parts", M)
    p, seed = 0.3, SEED_BIG
    results = []
    for fused in (False, True):
        part = nans((nparts + 1) * 2 * d)
        dx, dxd, dg, db = nans(M, d, dtype=dt, off=case.off), nans(M, d, dtype=dt, off=case.off), nans(d), nans(d)
        if fused:
            _lib.call("ka_tf_layernorm_bwd_drop", dyd, xd, gd, place(mean_in), place(rstd_in), drd, dx, dxd, p, seed, part, dg, db, M, d, code, st())
        else:
            _lib.call("ka_tf_layernorm_bwd", dyd, xd, gd, place(mean_in), place(rstd_in), drd, dx, part, dg, db, M, d, code, st())
        sync()
        results.append((dx.cpu(), dg.cpu(), db.cpu()))
        err = (dx.double().cpu() - ref["dx"]).abs()
        bound = th.ln_row_bound(ref["dx"], case.bf16)
        assert bool((err <= bound).all()), f"dx: worst {float((err / bound).max()):.2f} of the bound"
        for name, got in (("dgamma", dg), ("dbeta", db)):
            err, bound = (got.double().cpu() - ref[name]).abs(), M * 2.0 ** -23 * ref[name + "_abs"]
            print(f"{case.id} {name}: worst {float((err / bound.clamp_min(1e-300)).max()):.3f} of M 2^-23 sum |terms|")
            assert bool((err <= bound).all()), f"{name}: worst {float((err / bound.clamp_min(1e-300)).max()):.3f} of the bound"
        if fused:
            keep = th.keep_mask(seed, M * d, p).reshape(M, d)
            scaled = (dx.float().cpu() * torch.tensor(th.inv_keep(p), dtype=F32)).to(dt)
            assert torch.equal(dxd.cpu(), torch.where(keep, scaled, torch.zeros((), dtype=dt))), "dx_drop"
        else:
            assert bool(torch.isnan(dxd).all())
    assert all(torch.equal(a, b) for a, b in zip(*results)), "ka_tf_layernorm_bwd and _bwd_drop write the same dx, dgamma, dbeta"


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,d", [(1, 8), (3, 24), (33, 400)])
def test_add_pos_mean_pool_head_grad_exact(dt, B, d):
    """x[b, s] += row_embed[s / 9] + col_embed[s % 9]; pooled[b] = mean_s x[b, s] on multiples of 81; dx[b, s] = dpooled[b] / 81 +
    dflat[b, s] with either input null.  (33, 400): more than 4096 x 256 elements, the grid-stride loops iterate."""
    code, M = _lib.dtype_code(dt), B * S
    g = torch.Generator().manual_seed(B + d)
    x, rowe, cole = ints(g, M, d), ints(g, 9, d), ints(g, 9, d)
    xd = place(x, dt)
    _lib.call("ka_tf_add_pos", xd, place(rowe), place(cole), B, d, code, st())
    s = torch.arange(M) % S
    assert_same(xd, x.double() + rowe.double()[s // 9] + cole.double()[s % 9], "add_pos")
    x81 = 81.0 * ints(g, M, d)
    pooled = nans(B, d)
    _lib.call("ka_tf_mean_pool", place(x81, dt), pooled, B, d, code, st())
    assert_same(pooled, x81.double().reshape(B, S, d).sum(1) / 81.0, "mean_pool")
    dpooled, dflat = 81.0 * ints(g, B, d), ints(g, M, d)
    for use_p, use_f in ((True, True), (True, False), (False, True)):
        dx = nans(M, d, dtype=dt)
        _lib.call("ka_tf_head_grad", place(dpooled) if use_p else None, place(dflat, dt) if use_f else None, dx, B, d, code, st())
        want = (dpooled.double() / 81.0).repeat_interleave(S, 0) * use_p + dflat.double() * use_f
        assert_same(dx, want, f"head_grad pooled={use_p} flat={use_f}")


@pytest.mark.parametrize("M,N,nsplit", COLSUM_CASES)
def test_colsum_exact(M, N, nsplit):
    """out = the column sums, part[s] = those of row range s (ranges of ceil(M / nsplit) rows; trailing ones short or empty)."""
    g = torch.Generator().manual_seed(M + N)
    a = ints(g, M, N)
    for dt in (F32, BF16):
        part, out = nans(nsplit, N), nans(N)
        _lib.call("ka_tf_colsum", place(a, dt), part, out, M, N, nsplit, _lib.dtype_code(dt), st())
        assert_same(out, a.double().sum(0), "colsum")
        assert_same(part, torch.stack([a.double()[b:e].sum(0) for b, e in th.colsum_ranges(M, nsplit)]), "colsum parts")


@pytest.mark.parametrize("B", POS_GRAD_B)
def test_pos_grad_exact(B):
    """drow[r] = sum over boards and columns of dx[b, 9 r + c], dcol[c] likewise over rows: three launches, min(B, 64) board
    ranges (B = 65: two boards per range, 31 of the 64 ranges empty)."""
    d = 24
    g = torch.Generator().manual_seed(B)
    dx = ints(g, B * S, d)
    tot = dx.double().reshape(B, 9, 9, d).sum(0)
    for dt in (F32, BF16):
        scratch, drow, dcol = nans(65 * 81 * d), nans(9, d), nans(9, d)
        _lib.call("ka_tf_pos_grad", place(dx, dt), scratch, drow, dcol, B, d, _lib.dtype_code(dt), st())
        assert_same(drow, tot.sum(1), f"drow B={B}")
        assert_same(dcol, tot.sum(0), f"dcol B={B}")


@pytest.mark.parametrize("n", TANH_NS)
def test_tanh_and_its_backward(n):
    """tanh in place against fp64 to 2 ulp of fp32, tanh_bwd = dy (1 - y^2) to 1 ulp; n = 1024 * 256 + 1: the grid stride wraps."""
    g = torch.Generator().manual_seed(n)
    x, dy = 3 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    v = place(x)
    _lib.call("ka_tf_tanh", v, n, st())
    ref = torch.tanh(x.double())
    err = (v.double().cpu() - ref).abs() / th.ulp32(ref)
    print(f"tanh n={n}: worst {float(err.max()):.2f} ulp")
    assert float(err.max()) <= 2
    y = v.clone()
    dx = nans(n)
    _lib.call("ka_tf_tanh_bwd", place(dy), y, dx, n, st())
    ref = dy.double() * (1 - y.double().cpu() ** 2)
    err = (dx.double().cpu() - ref).abs() / th.ulp32(ref)
    print(f"tanh_bwd n={n}: worst {float(err.max()):.2f} ulp")
    assert float(err.max()) <= 1


@pytest.mark.parametrize("M,N,ldi,ldo,bf16", TRANSPOSE_CASES)
def test_transpose_pad_exact(M, N, ldi, ldo, bf16):
    """out[n][0:ldo] = bf16(in[0:M][n]) | 0: the 16-byte bf16 form (64 x 64 tiles, M and N no multiples of 64) and the scalar one."""
    dt = BF16 if bf16 else F32
    g = torch.Generator().manual_seed(M + N)
    x = th.padded(torch.randn(M, N, generator=g).to(dt).float(), ldi)
    out = nans(N, ldo, dtype=BF16)
    _lib.call("ka_tf_transpose_pad", place(x, dt), out, M, N, ldi, ldo, _lib.dtype_code(dt), st())
    want = torch.zeros(N, ldo, dtype=BF16)
    want[:, :M] = x[:, :N].t().bfloat16()
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("M,N,ldi,ldo,bf16", CAST_CASES)
def test_cast_pad_exact(M, N, ldi, ldo, bf16):
    dt = BF16 if bf16 else F32
    g = torch.Generator().manual_seed(M + N)
    x = th.padded(torch.randn(M, N, generator=g).to(dt).float(), ldi)
    out = nans(M, ldo, dtype=BF16)
    _lib.call("ka_tf_cast_pad", place(x, dt), out, M, N, ldi, ldo, _lib.dtype_code(dt), st())
    want = torch.zeros(M, ldo, dtype=BF16)
    want[:, :N] = x[:, :N].bfloat16()
    assert torch.equal(out.cpu(), want)
