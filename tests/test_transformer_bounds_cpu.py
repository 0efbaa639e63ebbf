"""The guard-band rig of tests/test_hip_conv_bounds.py and the cases of tests/test_hip_transformer_bounds.py, proved on the
CPU: the rig (with per-tensor guard-row counts) reports three torch-emulated faulty "kernels" -- a row written past the output,
a row read past the input, a valid element left unwritten -- each for the stated reason and passes a correct one; every case's
oracle data builds and takes the route it names; every guard is at least one workgroup span of its kernel and a multiple of 8
rows; and every ka_tf_* entry point that takes a tensor is named by a case."""
from pathlib import Path

import pytest
import torch

from keisei_amd import _lib
import transformer_helpers as th
from test_hip_conv_bounds import G, PATTERN, bits, check_guarded, guarded, guards_intact, middle, run_guarded

F32, BF16 = torch.float32, torch.bfloat16


def past(t, rows=1):
    """t with `rows` more rows of whatever lies behind it in its allocation: what a kernel without a bound sees."""
    return torch.as_strided(t, (t.shape[0] + rows, *t.shape[1:]), t.stride(), t.storage_offset())


def doubled(t):                                  # the correct "kernel": out = 2 x
    t["out"].copy_(2 * t["x"])


def writes_a_row_past_its_output(t):
    doubled(t)
    past(t["out"])[-1] = 7.0


def reads_a_row_past_its_input(t):
    doubled(t)
    t["out"][-1] += past(t["x"])[-1]


def result_depends_on_a_row_past_its_input(t):   # finite whatever lies there, but not the same
    doubled(t)
    t["out"][-1] += torch.isnan(past(t["x"])[-1]).to(t["out"].dtype)


def leaves_an_element_unwritten(t):
    keep = t["out"][1, 2].clone()
    doubled(t)
    t["out"][1, 2] = keep


FAULTS = ((writes_a_row_past_its_output, "guard rows overwritten"), (reads_a_row_past_its_input, "non-finite"),
          (result_depends_on_a_row_past_its_input, "depends on memory past the tensors"), (leaves_an_element_unwritten, "unwritten"))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("g", [None, 8, 256])
def test_rig_reports_each_emulated_fault(dt, g):
    x = torch.arange(15, dtype=torch.float32).reshape(5, 3).to(dt)
    ins = {"x": x} if g is None else {"x": (x, g)}
    outs = {"out": ((5, 3), dt)} if g is None else {"out": ((5, 3), dt, g)}
    m = check_guarded(doubled, ins, outs, device="cpu")
    assert torch.equal(m["out"], 2 * x)
    for kernel, reason in FAULTS:
        with pytest.raises(AssertionError, match=reason):
            check_guarded(kernel, ins, outs, device="cpu")
    # the same faults on a tensor updated in place
    for kernel, reason in ((lambda t: past(t["v"])[-1].fill_(1.0), "guard rows overwritten"),
                           (lambda t: t["v"][-1].add_(past(t["x"])[-1]), "non-finite")):
        with pytest.raises(AssertionError, match=reason):
            check_guarded(kernel, ins, {}, inout={"v": x if g is None else (x, g)}, device="cpu")
    m = check_guarded(lambda t: t["v"].mul_(2), {}, {}, inout={"v": x if g is None else (x, g)}, device="cpu")
    assert torch.equal(m["v"], 2 * x)


def test_rig_layout():
    """The default is G rows; a guard count and an element offset put the middle where they say, 16-byte aligned without the
    offset; guards_intact looks at every element outside the middle; the pattern is a NaN; `valid` cuts the pad columns out."""
    for dt in (F32, BF16):
        full, mid = guarded((3, 5), dt, "pattern", device="cpu")
        assert full.shape == (3 + 2 * G, 5) and mid.data_ptr() == full[G].data_ptr() and bool(torch.isnan(full).all())
        full, mid = guarded((3, 8), dt, "pattern", g=256, device="cpu")
        assert full.shape == (515, 8) and mid.data_ptr() == full[256].data_ptr() and (mid.data_ptr() - full.data_ptr()) % 16 == 0
        assert middle(full, 256).data_ptr() == mid.data_ptr() and middle(full, 256).shape == mid.shape
        for row in (0, 255, 259, 514):
            assert guards_intact(full, 256)
            saved = bits(full)[row, 7].clone()
            bits(full)[row, 7] = 0
            assert not guards_intact(full, 256)
            bits(full)[row, 7] = saved
        full, mid = guarded((11,), dt, "pattern", g=4096, off=1, device="cpu")
        assert full.shape == (11 + 8192 + 8,) and (mid.data_ptr() - full.data_ptr()) == (4096 + 1) * dt.itemsize
        assert middle(full, 4096, 1).data_ptr() == mid.data_ptr() and middle(full, 4096, 1).shape == (11,)
        for i in (4096, 4097 + 11, full.shape[0] - 1):                     # the elements right beside the middle are guards
            bits(full)[i] = 0
            assert not guards_intact(full, 4096, 1)
            bits(full)[i] = PATTERN[dt][1]
        mid.zero_()
        assert guards_intact(full, 4096, 1)
    fulls = run_guarded(lambda t: None, {"a": torch.ones(2, 2)}, {"o": ((2, 2), F32, 16)}, float("nan"), device="cpu")
    assert set(fulls) == {"o"} and fulls["o"].shape == (34, 2)

    def two_of_three_columns(t):
        t["out"][:, :2] = t["x"][:, :2]
    x = torch.ones(4, 3)
    with pytest.raises(AssertionError, match="non-finite"):
        check_guarded(two_of_three_columns, {"x": x}, {"out": ((4, 3), F32, 8)}, device="cpu")
    m = check_guarded(two_of_three_columns, {"x": x}, {"out": ((4, 3), F32, 8)}, valid={"out": lambda t: t[:, :2]}, device="cpu")
    assert bool((bits(m["out"])[:, 2] == PATTERN[F32][1]).all())


# ------------------------------------------------------------------------------------------------ the guards
def test_guards_cover_a_workgroup_span():
    """Section 1 of the rule: each guard is at least one whole tile or workgroup span along the guarded dimension, a multiple
    of 8 rows, and what the table of the issue says."""
    assert (th.BM, th.BN, th.K256_ROWS, th.BIG_M, th.BIG_N, th.TN_ROWS, th.TN_COLS, th.ATTN_PAIRS, th.SP) == (128, 128, 128, 256, 256, 64, 128, 4, 96)
    assert th.GUARD_ROWS == {"tiled": 256, "map": 256, "k256": 256, "big": 512, "tn": 256, "attn": 384}
    for kind, rows in th.GUARD_ROWS.items():
        assert rows >= th.SPAN[kind] and rows % 8 == 0, kind
    assert {c.form for c in th.NT_BOUNDS} == {"tiled", "map", "k256", "big"}
    for c in th.NT_BOUNDS:
        if len(c.ranges) > 1:                        # whole slabs of M rows on both sides of [ns][M][ldc]
            assert 8 * c.M >= th.GUARD_ROWS[c.form]
    for c in th.TN_BOUNDS:
        assert 8 * c.N >= th.GUARD_ROWS["tn"] and th.GUARD_FLAT >= th.TN_COLS
    for c in th.HOT_BOUNDS_REG + th.HOT_BOUNDS_LDS:
        assert th.lse_guard(c.H) == 4 * c.H * 96 and th.lse_guard(c.H) % 8 == 0
    for c in th.LN_BOUNDS:
        rows = th.ln_block_rows(c)
        L = th.ln_vec_lanes(c.d, c.bf16, not c.off)
        assert rows % 8 == 0 and rows >= 128 >= th.ceil_div(c.M, th.ln_parts(c.M)) and rows >= (16 * (64 // L) if L else 4)
        assert (th.ln_parts(c.M) * 2 * c.d) % 8 == 0 and (rows * c.d) % 8 == 0
    for cols in (1, 8, 24, 45, 255, 256, 257, 400):
        assert th.flat_rows(cols) % 8 == 0 and th.flat_rows(cols) * cols >= th.GUARD_FLAT
    assert th.GUARD_FLAT % 8 == 0 and all(th.round8(n) % 8 == 0 and 0 <= th.round8(n) - n < 8 for n in (1, 8, 765, 42120))


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", th.NT_BOUNDS, ids=[c.id for c in th.NT_BOUNDS])
def test_nt_bounds_case_builds_and_takes_its_route(case):
    d = th.nt_data(case)
    assert th.nt_route(case) == case.form and len(d.slabs) == len(case.ranges)
    assert case.K % 32 == 0 and case.lda % 8 == 0 and case.ldb % 8 == 0
    assert th.nt_partial_bound(case, d) < th.EXACT
    if case.c_bf16:
        assert torch.equal(d.slabs[0], d.slabs[0].float().bfloat16().double())


def test_nt_bounds_axes():
    t = th.NT_BOUNDS_TILED + th.NT_BOUNDS_LDS
    assert {c.M for c in t} == {1, 129} and {c.N for c in t} == {1, 130, 136} and {c.K for c in t} == {32, 96}
    scalar = lambda c: c.N % 4 or c.ldc % 4
    assert any(scalar(c) and not c.c_bf16 for c in t) and any(scalar(c) and c.c_bf16 for c in t)
    assert any(not scalar(c) and c.c_bf16 and not th.nt_lds_epilogue(c) for c in t), "8-byte stores"
    assert any(not scalar(c) and not c.c_bf16 for c in t), "16-byte stores"
    assert all(th.nt_lds_epilogue(c) and c.M % 128 for c in th.NT_BOUNDS_LDS) and not any(th.nt_lds_epilogue(c) for c in th.NT_BOUNDS_TILED)
    for bf in (False, True):
        assert {c.epi for c in t if c.c_bf16 == bf} >= {"none", "bias_relu", "bias_drop_res"}
    assert sum(c.masked for c in t) == 1
    assert all(len(c.ranges) > 1 for c in th.NT_BOUNDS_SPLIT) and all((c.M, c.N, c.K) == (897, 1025, 64) for c in th.NT_MAP)
    k = th.NT_BOUNDS_K256
    assert {c.M for c in k} == {1, 128, 129} and {c.N for c in k} == {64, 192} and {(c.M, c.N) for c in k} == {(m, n) for m in (1, 128, 129) for n in (64, 192)}
    assert {("res" in c.epi, c.masked) for c in k} == {(False, False), (True, False), (False, True)}
    assert {(c.M, c.N, c.K, c.epi, c.c_bf16) for c in th.NT_BOUNDS_BIG} == {(1025, 1027, 1088, "bias", False), (1025, 1027, 1088, "none", True)}


@pytest.mark.parametrize("case", th.TN_BOUNDS, ids=[c.id for c in th.TN_BOUNDS])
def test_tn_bounds_case_builds(case):
    d = th.tn_data(case)
    assert d.slabs.shape == (case.slabs, case.N, case.K) and d.colsum.shape == (case.slabs, case.N)
    assert th.tn_slabs(case.M, case.nsplit) == case.slabs


def test_tn_bounds_axes():
    assert [(c.M, c.N, c.K, c.slabs) for c in th.TN_BOUNDS] == [(1, 120, 264, 1), (65, 264, 120, 2), (4097, 136, 264, 4)]


def test_attention_bounds_cases_build_and_take_their_forms():
    reg, lds = th.HOT_BOUNDS_REG, th.HOT_BOUNDS_LDS
    assert [tuple(c) for c in reg] == [(1, 1, 8), (5, 1, 8), (3, 3, 16), (2, 5, 24), (1, 3, 32)]
    assert all(th.attn_register_form(True, c.H, c.dh, c.B) for c in reg) and {(c.B * c.H) % 4 for c in reg} == {1, 2, 3}
    assert {c.dh <= 16 for c in reg} == {True, False}, "both instantiations"
    assert {c.dh for c in lds} == {8, 40, 64}
    for c in lds:
        assert not th.attn_register_form(False, c.H, c.dh, c.B) and not th.attn_register_form(True, c.H, c.dh, c.B, lds_switch=True)
        assert (c.dh > 32) == (not th.attn_register_form(True, c.H, c.dh, c.B)), "dh = 40, 64: the LDS form without the switch"
    assert th.ATTN_BOUNDS_P == (0.0, 0.3, 0.5) and th.inv_keep(0.5) == 2.0 and th.inv_keep(0.3) not in (1.0, 2.0)
    for c in set(reg + lds):
        for many in (False, True):
            d = th.hot_data(c, many)
            out, dv = th.hot_ref(c, d)
            assert out.shape == dv.shape == (c.B * th.S, c.H * c.dh) and d.qkv.shape == (c.B * th.S, 3 * c.H * c.dh)
            f = th.hot_keep(c, d, th.SEED_BIG, 0.3)
            assert set(f.unique().tolist()) <= {0.0, th.inv_keep(0.3)} and bool((f == 0).any()) and bool((f != 0).any())


@pytest.mark.parametrize("case", th.LN_BOUNDS, ids=[c.id for c in th.LN_BOUNDS])
def test_layernorm_bounds_case_builds(case):
    x, gamma, beta, dy, dres = th.ln_data(case)
    ref = th.ln_ref(x, gamma, beta, dy, dres)
    assert ref["y"].shape == (case.M, case.d) and bool(torch.isfinite(ref["dx"]).all())


def test_layernorm_bounds_forms():
    lanes = {c: th.ln_vec_lanes(c.d, c.bf16, not c.off) for c in th.LN_BOUNDS}
    assert {(c.M, c.d) for c, L in lanes.items() if L == 32} == {(1, 256), (33, 256)} and {(c.M, c.d) for c, L in lanes.items() if L == 1} == {(1025, 8)}
    assert 16 * (64 // 32) == 32 and 16 * (64 // 1) == 1024, "rows per block of the 16-byte forward"
    for bf in (False, True):
        for d in (24, 400):
            assert {c.M for c, L in lanes.items() if L == 0 and c.d == d and c.bf16 == bf and not c.off} == {1, 5, 129}
    off = [c for c in th.LN_BOUNDS if c.off]
    assert len(off) == 1 and th.ln_vec_lanes(off[0].d, off[0].bf16) and lanes[off[0]] == 0
    assert [th.ln_parts(M) for M in (1, 128, 129, 1025, 10 ** 7)] == [1, 1, 2, 9, 2048]


def test_row_kernel_bounds_cases():
    assert th.W16_JOBS == ((8, 264), (139, 256), (70, 44))
    for N, K in th.W16_JOBS:
        W, out, outT = th.w16_data(N, K)
        assert K % 4 == 0 and out.shape == (N, th.w16_ld(K)) and outT.shape == (K, th.w16_ld(N)) and th.w16_ld(K) % 32 == 0
        assert torch.equal(out[:, :K].t(), outT[:, :N]) and not bool(out[:, K:].any()) and not bool(outT[:, N:].any())
    assert th.DROP_BOUNDS_NS == (1, 5, 1025) and th.ROW_BOUNDS == ((1, 8), (3, 24)) and th.POS_GRAD_BOUNDS_B == (1, 65)
    assert th.TANH_BOUNDS_NS == (1, 257)
    assert 1 + len(th.pos_grad_ranges(65)) == 65, "ka_tf_pos_grad: the result and one part per board range fill 65 * 81 * d floats"
    assert any(th.transpose_vec(*c) for c in th.TRANSPOSE_CASES) and any(not th.transpose_vec(*c) for c in th.TRANSPOSE_CASES)


# ------------------------------------------------------------------------------------------------ coverage
def test_every_entry_point_with_a_tensor_is_guarded():
    """Names from the library's signature table: every ka_tf_* function that takes a pointer besides its stream has cases, the
    GPU test calls it, and the only other ka_tf_* names are the route counters and the slab / part count queries."""
    tensors = {n for n, sig in _lib._SIGS.items() if n.startswith("ka_tf_") and sig.replace(" ", "")[:-1].count("p") > 0}
    others = {n for n in _lib._SIGS if n.startswith("ka_tf_")} - tensors
    assert others | {"ka_tf_route_counts"} == set(th.BOUNDS_NO_POINTERS_TO_GUARD)
    assert tensors - {"ka_tf_route_counts"} == set(th.BOUNDS_ENTRY_POINTS)
    gpu_test = (Path(__file__).parent / "test_hip_transformer_bounds.py").read_text()
    for name, cases in th.BOUNDS_ENTRY_POINTS.items():
        assert len(cases) > 0 and f'"{name}"' in gpu_test, name
