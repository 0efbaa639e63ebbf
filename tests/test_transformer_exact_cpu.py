"""The oracle of tests/test_hip_transformer_exact.py, proved on the CPU: the references of tests/transformer_helpers.py equal
plain torch (nn.functional.linear, autograd, layer_norm, softmax) bit for bit where exactness is claimed, in float32 too and with
the contraction walked backwards; every case's exactness and bf16-representability conditions hold; the restated launch rules
put every axis value on the route the case names; the dropout mask keeps 1 - p; and the comparison has teeth -- a reference
with one of the mistakes such a kernel can make fails torch.equal on every case the mistake applies to."""
import math

import pytest
import torch
import torch.nn.functional as F

import transformer_helpers as th
from transformer_helpers import (ATTN64_CASES, COLSUM_CASES, DROP_PS, EXACT, HOT_CASES, LN_CASES, MUTANTS, NT_BIG, NT_CASES, NT_K256,
                                 NT_LDS, NT_MAP, NT_SPLIT, NT_TILED, POS_GRAD_B, S, SEED_BIG, SEED_SMALL, TN_CASES, TRANSPOSE_CASES)

NT_IDS = [c.id for c in NT_CASES]


# ------------------------------------------------------------------------------------------------ the dropout mask
@pytest.mark.parametrize("p", DROP_PS)
def test_keep_mask_keeps_one_minus_p(p):
    for seed in (SEED_SMALL, SEED_BIG):
        kept = float(th.keep_mask(seed, 2 ** 20, p).double().mean())
        assert abs(kept - (1 - p)) < 0.01, (seed, kept)
    assert p > 0 or bool(th.keep_mask(SEED_BIG, 4096, p).all())


def test_keep_mask_is_the_scalar_rule():
    """The vectorised mask against the rule written out element by element on Python integers."""
    def hash32(x):
        x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ (x >> 16)
    idx = torch.tensor([0, 1, 2, 3, 1000, 1001, 2 ** 31 - 1, 2 ** 32 + 5, 2 ** 33 + 4])
    for seed in (SEED_SMALL, SEED_BIG):
        key = ((seed & 0xFFFFFFFF) * 0x9E3779B1 + (seed >> 32) * 0x85EBCA6B) & 0xFFFFFFFF
        for p in (0.1, 0.5):
            want = []
            for i in idx.tolist():
                pair = i >> 1
                h = hash32(((pair & 0xFFFFFFFF) * 0x9E3779B1 + (pair >> 32) * 0xC2B2AE35 + key) & 0xFFFFFFFF)
                want.append(((h >> 16) if i & 1 else (h & 0xFFFF)) >= int(p * 65536 + 0.5))
            assert th.keep_at(seed, idx, p).tolist() == want
    assert th.drop_thresh(0.1) == 6554 and th.drop_thresh(0.5) == 32768 and th.inv_keep(0.5) == 2.0
    assert not torch.equal(th.keep_mask(SEED_BIG, 4096, 0.5), th.keep_mask(SEED_BIG & 0xFFFFFFFF, 4096, 0.5)), "the high word enters"


# ------------------------------------------------------------------------------------------------ NT GEMM
@pytest.mark.parametrize("case", NT_CASES, ids=NT_IDS)
def test_nt_reference_equals_torch_bit_for_bit(case):
    d = th.nt_data(case)
    a, b = d.A[:, :case.K], d.B[:, :case.K]
    assert torch.equal(a, a.bfloat16().float()) and torch.equal(b, b.bfloat16().float()) and float(a.abs().max()) <= 2
    assert bool(torch.isnan(d.A[:, case.K:]).all()) and bool(torch.isnan(d.B[:, case.K:]).all())
    assert bool((a[:, -1] != 0).all()) and bool((b[:, -1] != 0).all()) and bool((a[-1] != 0).any())
    assert th.nt_partial_bound(case, d) < EXACT, "|partial sums| < 2^24 in any order"
    total = sum(d.slabs[1:], d.slabs[0])
    for dt in (torch.float64, torch.float32):
        got = F.linear(a.to(dt), b.to(dt), None if d.bias is None else d.bias.to(dt))
        flipped = F.linear(a.flip(1).to(dt), b.flip(1).to(dt), None if d.bias is None else d.bias.to(dt))
        assert torch.equal(got, flipped), "the same sum, K walked backwards"
        if len(d.slabs) > 1:
            assert torch.equal(got.double(), total)
            for (kb, ke), slab in zip(case.ranges, d.slabs):
                assert torch.equal(slab, (a[:, kb:ke].to(dt) @ b[:, kb:ke].to(dt).t()).double())
            continue
        v = torch.relu(got) if "relu" in case.epi else got
        if case.p:
            keep = th.keep_mask(d.seed, case.M * case.ldc, case.p).reshape(case.M, case.ldc)[:, :case.N]
            v = v * keep * 2
        if d.act is not None:
            v = v * (d.act[:, :case.N] > 0)
        if d.res is not None:
            v = v + d.res[:, :case.N].to(dt)
        assert torch.equal(v.double(), total), dt
    if case.c_bf16:
        assert torch.equal(total, total.float().bfloat16().double()), "every bf16 output exactly representable"
    floor = 0.08 if case.p and ("relu" in case.epi or case.masked) else 0.15          # (ReLU and p = 0.5 leave a quarter)
    assert float((total != 0).double().mean()) > floor or case.M * case.N < 16, "an output of zeros would hide a dropped product"
    if d.act is not None:
        z = d.act[:, :case.N]
        assert case.M * case.N < 64 or (bool(((z == 0) & torch.signbit(z)).any()) and bool(((z == 0) & ~torch.signbit(z)).any()))


def test_nt_ranges_and_routes():
    """The restated rules put every case on the route it names and every axis value of the issue on the tiled kernel."""
    for c in NT_CASES:
        assert th.nt_route(c) == c.form, c.id
        assert c.K % 32 == 0 and c.lda % 8 == 0 and c.ldb % 8 == 0
        if c.form == "k256":
            assert th.nt_route(c, k256=False) == "tiled"
        if c.form == "big":
            assert th.nt_route(c, big=False) in ("map", "tiled")
    tiled = [c for c in NT_TILED]
    assert {c.M for c in tiled} == {1, 127, 128, 129, 257} and {c.N for c in tiled} == {1, 3, 4, 7, 8, 127, 128, 136, 139}
    assert {c.K for c in tiled} == {32, 64, 96, 2592} and {c.lda_pad for c in tiled} == {0, 8} == {c.ldb_pad for c in tiled}
    assert {c.ldc_pad for c in tiled} == {0, 1, 4, 8}
    for bf in (False, True):
        epis = {c.epi for c in tiled if c.c_bf16 == bf}
        assert epis == set(th.EPILOGUES) - (set() if bf else set(th.MASKED))
        for n in (1, 3, 4, 7, 8, 127, 128, 136, 139):
            assert {c.epi for c in tiled if c.c_bf16 == bf and c.N == n} == epis
    for c in tiled:                                   # every dropout case at two ldc
        if c.p:
            assert len({o.ldc for o in tiled if o._replace(ldc_pad=0) == c._replace(ldc_pad=0)}) == 2, c.id
    assert {c.epi for c in NT_LDS} == set(th.EPILOGUES) and all(th.nt_lds_epilogue(c) and (c.M % 128 or c.N % 128) for c in NT_LDS)
    # split K: the slab counts, a short last range, fewer slabs than asked for
    assert [(c.nsplit, th.nt_slabs(c.K, c.nsplit)) for c in NT_SPLIT] == [(2, 2), (2, 1), (3, 3), (3, 2), (8, 5), (8, 7)]
    assert {c.nsplit for c in NT_SPLIT} == {2, 3, 8}
    for c in NT_SPLIT:
        r = c.ranges
        assert r[0][0] == 0 and r[-1][1] == c.K and all(x[1] == y[0] for x, y in zip(r, r[1:])) and all(e > b for b, e in r)
    assert any(len(c.ranges) > 1 and c.ranges[-1][1] - c.ranges[-1][0] < c.ranges[0][1] for c in NT_SPLIT)
    assert all(math.ceil(c.N / 128) > 8 and math.ceil(c.M / 128) >= 8 for c in NT_MAP) and (897, 1025, 64) == NT_MAP[0][1:4]
    assert {c.M for c in NT_K256} == {1, 127, 128, 129, 300} and {c.N for c in NT_K256} == {64, 128, 272, 1024}
    assert all((c.form == "tiled") == (c.N == 272) for c in NT_K256)
    k = [c for c in NT_K256 if c.form == "k256"]
    assert {("res" in c.epi, c.masked) for c in k} == {(False, False), (True, False), (False, True)}     # (both: not reachable from the C ABI)
    assert {c.ldc_pad for c in k} == {0, 8} and {c.lda_pad for c in k} == {0, 8} == {c.ldb_pad for c in k}
    assert {(c.M, c.N, c.K) for c in NT_BIG if c.form == "big"} == {(1024, 1024, 1024), (1025, 1027, 1088), (1281, 2305, 1024)}
    assert all(c.ldc % 8 == 0 for c in NT_BIG if c.c_bf16) and any(c.K == 1056 and c.form != "big" for c in NT_BIG)


# ------------------------------------------------------------------------------------------------ TN GEMM
@pytest.mark.parametrize("case", TN_CASES, ids=[c.id for c in TN_CASES])
def test_tn_reference_equals_autograd_bit_for_bit(case):
    d = th.tn_data(case)
    a, b = d.A[:, :case.N], d.B[:, :case.K]
    assert th.tn_slabs(case.M, case.nsplit) == case.slabs == len(case.ranges) and case.ranges[-1][1] == case.M
    assert all(e > b_ for b_, e in case.ranges) and bool(torch.isnan(d.A[:, case.N:]).all()) and bool(torch.isnan(d.B[:, case.K:]).all())
    for dt in (torch.float64, torch.float32):
        W = torch.zeros(case.N, case.K, dtype=dt, requires_grad=True)
        bias = torch.zeros(case.N, dtype=dt, requires_grad=True)
        F.linear(b.to(dt), W, bias).backward(a.to(dt))
        assert torch.equal(W.grad.double(), d.slabs.sum(0)) and torch.equal(bias.grad.double(), d.colsum.sum(0))
        assert torch.equal(W.grad, a.flip(0).to(dt).t() @ b.flip(0).to(dt)), "the same sum, tokens walked backwards"
    assert case.N % 8 == 0 and case.K % 8 == 0 and case.lda % 8 == 0 and case.ldb % 8 == 0


def test_tn_axes():
    assert {c.slabs for c in TN_CASES} >= {1, 2, 7, 8, 9, 16, 17} and {c.M for c in TN_CASES} >= {1, 63, 64, 65, 4097}
    assert {c.N for c in TN_CASES} == {8, 120, 128, 136, 264} == {c.K for c in TN_CASES}
    assert {c.ldc_pad for c in TN_CASES} == {0, 4, 1} and any(c.lda_pad for c in TN_CASES) and any(c.ldb_pad for c in TN_CASES)
    assert any(c.K > 128 and c.slabs > 1 for c in TN_CASES), "column sums beside more than one k-tile"


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("case", HOT_CASES, ids=[c.id for c in HOT_CASES])
@pytest.mark.parametrize("many", [False, True])
def test_one_hot_construction(case, many):
    """The softmax of the constructed scores is exactly one-hot in fp32 (every other exp underflows to 0) and selects with
    probability exactly 1 in fp64, where the other probabilities stay below 2^-172 = exp(-120): they vanish from any fp32 or
    bf16 product.  out and dV of the reference equal autograd on that softmax."""
    d = th.hot_data(case, many)
    B, H, dh = case
    assert dh >= 8 and torch.equal(d.qkv, d.qkv.bfloat16().float()) and torch.equal(d.dout, d.dout.bfloat16().float())
    s = th.hot_scores(case, d)
    onehot = F.one_hot(d.phi, S).double()
    assert torch.equal(s.argmax(-1), d.phi) and float(s.max()) == d.smax == float(s.amax(-1).min())
    second = s.masked_fill(onehot.bool(), -1e30).amax(-1)
    scale = 1.0 / math.sqrt(dh)
    assert float(((s.amax(-1) - second) * scale).min()) > 120
    sel = torch.tensor(d.smax, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32)          # fp32 scale, fp32 product
    assert math.log2(d.smax).is_integer() and float(sel.double()) == d.smax * float(torch.tensor(scale, dtype=torch.float32)), "exact"
    assert torch.equal(torch.softmax(s.float() * scale, -1), onehot.float())
    p64 = torch.softmax(s * scale, -1)
    assert torch.equal(p64 * onehot, onehot) and float((p64 * (1 - onehot)).max()) < 2.0 ** -172
    assert torch.allclose(torch.logsumexp(s.float() * scale, -1).double(), s.amax(-1) * scale, rtol=1e-6, atol=0)
    assert (sorted(d.phi[0, 0].tolist()) == list(range(S))) != many
    # the reference against autograd through the exact one-hot probabilities
    dm = H * dh
    v = d.qkv[:, 2 * dm:].double().requires_grad_(True)
    out = (onehot @ th.heads_of(v, B, H, dh)).transpose(1, 2).reshape(B * S, dm)
    out.backward(d.dout.double())
    ref_out, ref_dv = th.hot_ref(case, d)
    assert torch.equal(out.detach(), ref_out) and torch.equal(v.grad, ref_dv)
    for p in (0.0, 0.5):
        o, dv = th.hot_ref(case, d, SEED_BIG, p)
        assert torch.equal(o, o.float().bfloat16().double()) and torch.equal(dv, dv.float().bfloat16().double())
        f = th.hot_keep(case, d, SEED_BIG, p)
        assert p == 0 or B * H * S < 200 or (0.3 < float((f == 0).double().mean()) < 0.7 and set(f.unique().tolist()) == {0.0, 2.0})


def test_attention_routes():
    assert {(c.H, c.dh) for c in HOT_CASES} == {(1, 8), (3, 16), (5, 24), (8, 32), (3, 40), (2, 48), (1, 56), (2, 64)}
    reg = [c for c in HOT_CASES if th.attn_register_form(True, c.H, c.dh, c.B)]
    assert {c.dh for c in reg} == {8, 16, 24, 32} and {(c.B * c.H) % 4 for c in reg} == {0, 1, 2, 3} and any(c.B * c.H == 1 for c in reg)
    assert not any(th.attn_register_form(False, c.H, c.dh) or th.attn_register_form(True, c.H, c.dh, lds_switch=True) for c in HOT_CASES)
    assert {dh for bf, _, dh, _ in ATTN64_CASES if bf} == {16, 24, 40, 48, 56} and {dh for bf, _, dh, _ in ATTN64_CASES if not bf} == {4, 12, 40, 64}
    assert {dh for bf, H, dh, B in ATTN64_CASES if th.attn_register_form(bf, H, dh, B)} == {16, 24}


@pytest.mark.parametrize("bf16,H,dh,B", ATTN64_CASES)
def test_attention_reference_equals_autograd(bf16, H, dh, B):
    """attn_ref64 without the emulation is softmax attention and its autograd gradient, to fp64 rounding; with it, it moves by
    about the bf16 spacing and no more."""
    qkv, dout = th.attn64_data(bf16, H, dh, B)
    d = H * dh
    x = qkv.double().requires_grad_(True)
    q, k, v = (th.heads_of(t, B, H, dh) for t in (x[:, :d], x[:, d:2 * d], x[:, 2 * d:]))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    out = torch.softmax(sc, -1) @ v
    out.backward(th.heads_of(dout.double(), B, H, dh))
    g = [th.heads_of(t, B, H, dh) for t in (x.grad[:, :d], x.grad[:, d:2 * d], x.grad[:, 2 * d:])]
    ref = th.attn_ref64(qkv, dout, B, H, dh)
    for got, want in zip((out.detach(), torch.logsumexp(sc, -1).detach(), *g), ref):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-12)
    for from_out in (False, True):
        emu = th.attn_ref64(qkv, dout, B, H, dh, emulate=True, d_from_out=from_out)
        for i in (0, 2, 3, 4):
            e = float(th.rel_l2(emu[i], ref[i], (0, 1, 2, 3)))
            assert 2.0 ** -11 < e < 2.0 ** -6, (i, e)


# ------------------------------------------------------------------------------------------------ LayerNorm, row kernels
@pytest.mark.parametrize("case", LN_CASES, ids=[c.id for c in LN_CASES])
def test_layernorm_reference_equals_torch(case):
    x, gamma, beta, dy, dres = th.ln_data(case)
    ref = th.ln_ref(x, gamma, beta, dy, dres)
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(xr, (case.d,), gr, br, th.LN_EPS)
    y.backward(dy.double())
    dx = xr.grad + (dres.double() if dres is not None else 0)
    tol = dict(rtol=1e-9, atol=1e-9) if not case.far else dict(rtol=1e-6, atol=1e-6)
    assert torch.allclose(y.detach(), ref["y"], **tol) and torch.allclose(dx, ref["dx"], **tol)
    assert torch.allclose(gr.grad, ref["dgamma"], **tol) and torch.allclose(br.grad, ref["dbeta"], **tol)
    dt = torch.bfloat16 if case.bf16 else torch.float32
    assert torch.equal(x, x.to(dt).float()) and (not case.far or abs(float(x.mean()) - 1000) < 2)


def test_layernorm_routes():
    for bf16, ds, vec in ((True, (8, 16, 24, 128, 256, 512, 520), {8: 1, 16: 2, 128: 16, 256: 32, 512: 64}),
                          (False, (4, 12, 64, 256, 260), {4: 1, 64: 16, 256: 64})):
        mine = [c for c in LN_CASES if c.bf16 == bf16]
        assert {c.d for c in mine} == set(ds) and {c.M for c in mine} == {1, 3, 127, 128, 129, 1000}
        assert {d: th.ln_vec_lanes(d, bf16) for d in ds if th.ln_vec_lanes(d, bf16)} == vec
        assert any(c.off and th.ln_vec_lanes(c.d, bf16) and not th.ln_vec_lanes(c.d, bf16, aligned=False) for c in mine)
        assert any(c.far for c in mine) and any(not c.dres and th.ln_vec_lanes(c.d, bf16) for c in mine) and \
            any(not c.dres and not th.ln_vec_lanes(c.d, bf16) for c in mine)
        for d in ds:
            assert {c.M for c in mine if c.d == ds[3]} == {1, 3, 127, 128, 129, 1000}


def test_row_kernel_rules():
    # mean over 81 squares of multiples of 81, as the kernels compute it (fp32 sum times fp32 1 / 81), is the exact integer
    k = torch.arange(-2 * 81, 2 * 81 + 1, dtype=torch.float32)
    assert torch.equal((k * 81) * torch.tensor(1.0 / 81.0, dtype=torch.float32), k)
    x = 81.0 * torch.arange(-2, 3)
    assert torch.equal(x, x.bfloat16().float()), "the inputs 81 * (-2..2) fit bf16"
    r = th.pos_grad_ranges(65)
    assert len(r) == 64 and sum(e > b for b, e in r) == 33 and r[-1] == (65, 65), "B = 65: half of the ranges are empty"
    assert all(len(th.pos_grad_ranges(B)) == min(B, 64) and th.pos_grad_ranges(B)[-1][1] == B for B in POS_GRAD_B)
    assert {ns for _, _, ns in COLSUM_CASES} == {1, 3, 8} and {M for M, _, _ in COLSUM_CASES} == {1, 80, 81, 4097}
    assert {N for _, N, _ in COLSUM_CASES} == {1, 255, 256, 257}
    assert any(th.transpose_vec(*c) and c[0] % 64 and c[1] % 64 and c[3] > c[0] for c in TRANSPOSE_CASES)
    assert any(not th.transpose_vec(*c) and c[4] for c in TRANSPOSE_CASES) and any(not c[4] for c in TRANSPOSE_CASES)
    u = th.ulp32(torch.tensor([1.0, 1.5, 0.75, 3.0], dtype=torch.float64))
    assert u.tolist() == [2.0 ** -23, 1.5 * 2.0 ** -23, 0.75 * 2.0 ** -23, 3 * 2.0 ** -23]


# ------------------------------------------------------------------------------------------------ the comparison has teeth
@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_wrong_reference_fails_on_every_case_it_applies_to(name):
    checked = 0
    for passes, cases in MUTANTS[name]:
        assert len(cases) > 0
        for c in cases:
            assert not passes(c), f"{name} passes on {getattr(c, 'id', c)}"
            checked += 1
    assert checked > 0
