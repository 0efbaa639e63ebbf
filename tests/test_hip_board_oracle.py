"""The board kernels (csrc/board.hip) against the float64 oracle of tests/board_helpers.py, form by form.

Every case asserts the kernel form it runs (ka_board_form and the `supported` queries against the Python mirror), hands the
library NaN-prefilled outputs and holds each output tensor to MARGIN x e32 [+ 2**-8 |ref| where it is stored in bf16], to
equality (max, ties, the layout kernels, the integer reductions) or to one float32 ulp (coefficients that are one rounding of
a float64 value).  Statistics are taken over the kernel's own stored `out`, the tail of a fused boundary launch over its own
stored dx / du: each stage is checked apart and is an exact input of the next.  B = 3: board 1 carries the edge planes.

The <11, 256> instantiations of the 16-byte kernels cannot be reached (a 256-thread shape has at most 16 channel pieces, hence
at most 6 squares per thread: test_board_oracle_cpu.py::test_case_forms_are_the_ones_named) and are not tried.

Forms per entry point (asserted by each case through ka_board_form / the `supported` queries):
  ka_block_tail_fwd, ka_pool_fwd   16-byte <6,256> <6,512> <11,512> (bf16 C = 512, f32 C = 256), KA_TAIL_FWD_KB = 2 / 3 / 6;
                                   channel pairs at C = 6, 48, 96, two passes at C = 512, KA_BOARD_PAIRS at C = 256 / 512;
                                   with / without se, res, pool; all-negative, constant, all-zero and tied planes
  ka_block_tail_fwd_se             every supported (C, H), H = 2 included, b1 / b2 given and NULL; refusals write nothing
  ka_block_dx                      16-byte 256 / 512 threads (21 squares at f32 C = 512), pairs; with / without dxc, dout / out
  ka_tail_bwd_reduce, _dz          pairs at C = 6, 32, 96, 256, 512 (two passes)
  ka_tail_bwd_fused                <6,256> <6,512> <11,512> in both dtypes, FC weights pre-loaded and rolled (H = 32, 64; bf16 C = 512)
  ka_block_dx_tail_bwd, _du        every supported pair of that list; dxc NULL; the heads form
  ka_block_dx_tail_bwd_du_gate     the same, batched (H % 4 == 0) and un-batched loops, KA_TAIL_GATE_P4 = 0 and 1 (half-width pieces)
  the three fused entry points     C = 8..512 step 8 x H = 1..64 x both dtypes at B = 1: launches and meets the oracle, or fails and writes nothing
  ka_relu_bn_bwd_reduce, ka_bn_bwd_apply      pairs at C = 6, 96, 128, 512 (two passes), placed exact zeros
  ka_bn_reduce, ka_pair_reduce, ka_sync_reduce, ka_bn_reduce_coeffs, ka_pair_reduce_bwd_coeffs, ka_bn_coeffs_parts,
  ka_bn_bwd_coeffs_parts           every loop edge of colsum2_stage1_body, unequal row counts, exact integer sums
  ka_bn_coeffs, ka_bn_bwd_coeffs, ka_bn_eval_coeffs[_multi], ka_affine_rows, ka_obs_to_nhwc, ka_nhwc_to_nchw      their arguments

Mutants and the tests whose reference carries them (board_helpers.FAMILIES): board_row -> test_forward_tail_pool_and_block_dx,
test_forward_tail_with_the_se_chain_inside, test_two_launch_tail_backward, test_single_pass_tail_backward,
test_block_boundary_launches; std_corr1, sq80_twice -> test_forward_tail_pool_and_block_dx (pool), sq80_twice also the tail and
relu tests; dsq81, sig_not_dsig, s2_no_addSy -> test_two_launch_tail_backward, test_single_pass_tail_backward,
test_block_boundary_launches; dh_mask -> the latter two; mask_ge -> those three, test_forward_tail_pool_and_block_dx (block_dx)
and test_relu_bn_backward_and_bn_apply; max_not_div, max_first, std_nozero -> test_forward_tail_pool_and_block_dx,
test_block_boundary_launches; du_up_remask -> test_block_boundary_launches; k2 -> test_relu_bn_backward_and_bn_apply;
rv_biased, eval_k -> test_bn_coefficient_arguments, test_reducers_equal_exact_integer_sums.

Measured on an MI355X: 174 test cases (each grid test walks 448 shapes x 3 entry points), the whole file 7.0 s wall, no test
above 2 s, peak device memory 20 MiB.  Worst error / bound: every output stored in bf16 reaches 0.99 (the 2**-8 |ref| term IS
the rounding of a value just above a power of two); fp32 outputs stay below 0.5 except se1 of the SE chain inside the forward
tail (0.65 at f32 C = 256, H = 4: 12 elements) and dh of the grid (0.59 at f32 C = 256, H = 2: 2 elements) -- tensors so small
that e32, a maximum over their elements, is a few draws; coefficients that are one rounding of float64 are within 0.5 ulp.
No kernel defect was found.  One documented relation was narrower than written: with the half-width pieces (KA_TAIL_GATE_P4, the
default at bf16 C = 256) dse / dh / s1 / s2 of the gate form equal the chain form's to rounding, not to the bit (du does).
"""
import math

import pytest
import torch

import board_helpers as bh
from board_helpers import DT, CODE, F32, F64
from keisei_amd import _lib
from keisei_amd._lib import KeiseiHipError
from test_hip_conv_bounds import check_guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
WORST = {}                                       # (family, tensor) -> (ratio, case): printed when the module is done


def st():
    return _lib.stream_ptr()


def act(t, dtn):
    return t.to(DT[dtn]).to(DEV).contiguous()


def vec(t):
    return t.float().to(DEV).contiguous()


def nans(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def back(t):
    return t.detach().double().cpu()


@pytest.fixture(scope="module", autouse=True)
def report():
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\npeak device memory {torch.cuda.max_memory_allocated() / 2 ** 20:.1f} MiB; worst error / bound per output tensor")
    for (fam, k), (r, case) in sorted(WORST.items()):
        print(f"  {fam:28s} {k:8s} {r:8.4f}  at {case}" + ("   <-- above 0.5" if r > 0.5 else ""))


def hold(fam, case, fn, c, got, act_names=(), exact=(), alg=False, bound=None, **kw):
    """every tensor of `got` against fn's float64 run; the fp32 run of the same formulas sets the bound.  bound = (fn, case):
    e32 is the larger of this case's and that case's (the one-board launches of the grid: see test_supported_implies_it_launches)"""
    r64, r32 = fn(c, F64, **kw), fn(c, F32, alg=alg, **kw)
    e32 = None
    if bound is not None:
        b64, b32 = bound[0](bound[1], F64), bound[0](bound[1], F32, alg=alg)
        e32 = {k: max(bh.e32_of(b32[k].double(), b64[k].double()), bh.e32_of(r32[k].double(), r64[k].double())) for k in got if k not in exact}
    r = bh.judge({k: back(v) for k, v in got.items()}, r64, r32, {k: DT[c["dtn"]] for k in act_names}, exact, e32)
    for k, v in r.items():
        if v >= WORST.get((fam, k), (-1.0, None))[0]:
            WORST[(fam, k)] = (v, case)
    assert max(r.values()) <= 1.0, f"{fam} {case}: error / bound {r}"
    return r


def form_is(kernel, C, H, dtn, pairs=False, p4=True):
    f = bh.board_form(kernel, C, H, dtn, pairs, p4)
    assert _lib.query("ka_board_form", kernel, C, H, CODE[dtn]) == bh.encode_form(f), (kernel, C, H, dtn, f)
    return f


def fails_and_writes_nothing(name, args, outs):
    with pytest.raises(KeiseiHipError):
        _lib.call(name, *args)
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o.float()).all()), f"{name}: an unsupported shape wrote something"


# ------------------------------------------------------------------------------------------------ forward tail, pool, block_dx


def run_tail_fwd(c, dtn, use_se, use_res, want_pool):
    Bn, C = c["B"], c["C"]
    out, pool = nans((Bn, 81, C), DT[dtn]), nans((Bn, 4 * C))
    _lib.call("ka_block_tail_fwd", act(c["y"], dtn), vec(c["scale"]), vec(c["shift"]), vec(c["se"]) if use_se else None,
              act(c["res"], dtn) if use_res else None, out, pool if want_pool else None, Bn, C, CODE[dtn], st())
    torch.cuda.synchronize()
    return out, pool


def hold_pool(fam, case, c, x_stored, pool):
    C = c["C"]
    hold(fam, case, bh.fam_pool, c, bh._split_pool(pool, C), exact=("max", "ties"), x=back(x_stored))


@pytest.mark.parametrize("C,dtn,pairs", list(bh.FWD_CASES), ids=lambda v: str(v))
def test_forward_tail_pool_and_block_dx(ka_env, C, dtn, pairs):
    """ka_block_tail_fwd (with / without se, res, pool; the KA_TAIL_FWD_KB forms), ka_pool_fwd, ka_block_dx (with / without dxc,
    dout / out) in the 16-byte forms, the channel-pair forms (C = 6, 48, 96; one and two passes) and under KA_BOARD_PAIRS"""
    if pairs:
        ka_env.set("KA_BOARD_PAIRS", "1")
    named = bh.FWD_CASES[(C, dtn, pairs)]
    assert form_is(0, C, 0, dtn, pairs)[:len(named)] == named
    fdx = form_is(1, C, 0, dtn, pairs)
    assert fdx[0] == ("pair" if pairs or bh.board16_plan(C, dtn) is None else "p16")      # (ka_block_dx has no square limit)
    c = bh.act_case(C, dtn)
    case = f"C={C} {dtn}" + (" pairs" if pairs else "")
    base = None
    for use_se, use_res, want_pool in ((True, True, True), (True, False, True), (False, True, True), (False, False, False)):
        out, pool = run_tail_fwd(c, dtn, use_se, use_res, want_pool)
        hold("tail_fwd", case, bh.fam_tail_fwd(use_se, use_res), c, {"out": out}, act_names=("out",))
        for kind, (b, ch) in c["slots"].items():                       # the edge planes arrive in `out` to the bit
            assert torch.equal(back(out[b, :, ch]), torch.relu(c["x"][b, :, ch])), (kind, use_se, use_res)
        if want_pool:
            hold_pool("tail_fwd pool", case, c, out, pool)
        else:
            assert bool(torch.isnan(pool).all())
        if use_se and use_res:
            base = (out, pool)
    if named == ("p16", 512, 6):
        for kb in ("2", "3", "6"):
            ka_env.set("KA_TAIL_FWD_KB", kb)
            out, pool = run_tail_fwd(c, dtn, True, True, True)
            assert torch.equal(out, base[0]) and torch.equal(pool, base[1]), kb
        ka_env.unset("KA_TAIL_FWD_KB")
    # ka_pool_fwd: the raw statistics of x (all-negative plane included)
    pool = nans((c["B"], 4 * C))
    _lib.call("ka_pool_fwd", act(c["x"], dtn), pool, c["B"], C, CODE[dtn], st())
    torch.cuda.synchronize()
    hold_pool("pool_fwd", case, c, c["x"], pool)
    for kind, (b, ch) in c["slots"].items():
        assert float(pool[b, 3 * C + ch]) == bh.EDGE_TIES[kind], kind
    # ka_block_dx
    for use_dxc, up in ((True, "masked"), (False, "none"), (True, "none"), (False, "masked")):
        dx = nans((c["B"], 81, C), DT[dtn])
        _lib.call("ka_block_dx", act(c["dxc"], dtn) if use_dxc else None, act(c["dout_up"], dtn) if up == "masked" else None,
                  act(c["out_up"], dtn) if up == "masked" else None, act(c["x"], dtn), vec(c["xpool"]), vec(c["dpool"]), dx,
                  c["B"], C, CODE[dtn], st())
        torch.cuda.synchronize()
        hold("block_dx", case, bh.fam_block_dx(use_dxc, up), c, {"dx": dx}, act_names=("dx",))


SE_GRID = [(C, H, dtn) for dtn in ("bf16", "f32") for C in bh.ACT_C[dtn] for H in bh.SE_H]


@pytest.mark.parametrize("C,H,dtn", SE_GRID, ids=lambda v: str(v))
def test_forward_tail_with_the_se_chain_inside(C, H, dtn):
    """ka_block_tail_fwd_se wherever its query says 1 (H < 4 included), b1 / b2 given and NULL: sqz, se1, se against the chain's
    reference, out against the tail on the launch's own se and bit for bit the plain launch; where the query says 0 (it must say
    so exactly where the mirror does) the call fails and writes nothing"""
    ok = bh.fwd_se_supported(C, H, dtn)
    assert bool(_lib.query("ka_block_tail_fwd_se_supported", C, H, CODE[dtn])) == ok
    c = bh.act_case(C, dtn, H)
    Bn, case = c["B"], f"C={C} H={H} {dtn}"
    for bias in (True, False):
        out, pool = nans((Bn, 81, C), DT[dtn]), nans((Bn, 4 * C))
        sqz, se1, se = nans((Bn, C)), nans((Bn, H)), nans((Bn, 2 * C))
        args = (act(c["y"], dtn), vec(c["scale"]), vec(c["shift"]), vec(c["bsum"]), vec(c["W1"]), vec(c["b1"]) if bias else None,
                vec(c["W2"]), vec(c["b2"]) if bias else None, act(c["res"], dtn), out, pool, sqz, se1, se, Bn, C, H, CODE[dtn], st())
        if not ok:
            fails_and_writes_nothing("ka_block_tail_fwd_se", args, (out, pool, sqz, se1, se))
            continue
        assert form_is(0, C, 0, dtn)[0] == "p16"
        _lib.call("ka_block_tail_fwd_se", *args)
        torch.cuda.synchronize()
        hold("tail_fwd_se chain", case, bh.fam_se_chain(bias), c, {"sqz": sqz, "se1": se1, "se": se})
        hold("tail_fwd_se", case, lambda cc, dt, mutant=None, alg=False: {"out": bh.ref_tail_fwd(cc, dt, se=back(se))}, c,
             {"out": out}, act_names=("out",))
        hold_pool("tail_fwd_se pool", case, c, out, pool)
        out2, pool2 = nans((Bn, 81, C), DT[dtn]), nans((Bn, 4 * C))
        _lib.call("ka_block_tail_fwd", act(c["y"], dtn), vec(c["scale"]), vec(c["shift"]), se, act(c["res"], dtn), out2, pool2, Bn, C,
                  CODE[dtn], st())
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(pool, pool2)


# ------------------------------------------------------------------------------------------------ tail backward


@pytest.mark.parametrize("C,dtn", bh.act_cases(bh.PAIR_KERNEL_C), ids=lambda v: str(v))
def test_two_launch_tail_backward(C, dtn):
    """ka_tail_bwd_reduce and ka_tail_bwd_dz (channel-pair kernels at every C; two passes at C = 512)"""
    pf = bh.pair_form(C)
    assert pf is not None and pf[3] == (2 if C == 512 else 1)
    c = bh.act_case(C, dtn)
    Bn = c["B"]
    dse, dz, s1, s2 = nans((Bn, 2 * C)), nans((Bn, 81, C), DT[dtn]), nans((Bn, C)), nans((Bn, C))
    dout, out, y, se = act(c["dout"], dtn), act(c["x"], dtn), act(c["y"], dtn), vec(c["se_bwd"])
    _lib.call("ka_tail_bwd_reduce", dout, out, y, vec(c["scale"]), vec(c["shift"]), se, dse, Bn, C, CODE[dtn], st())
    _lib.call("ka_tail_bwd_dz", dout, out, y, se, vec(c["dsq"]), vec(c["mean"]), vec(c["invstd"]), dz, s1, s2, Bn, C, CODE[dtn], st())
    torch.cuda.synchronize()
    hold("tail_unfused", f"C={C} {dtn}", bh.fam_tail_unfused, c, {"dse": dse, "dz": dz, "s1": s1, "s2": s2}, act_names=("dz",))


def tail_operands(c, dtn):
    return (act(c["y"], dtn), vec(c["scale"]), vec(c["shift"]), vec(c["se_bwd"]), vec(c["se1"]), vec(c["W2"]), vec(c["W1"]),
            vec(c["mean"]), vec(c["invstd"]))


def tail_outs(c, dtn):
    Bn, C, H = c["B"], c["C"], c["H"]
    return {"dz": nans((Bn, 81, C), DT[dtn]), "dse": nans((Bn, 2 * C)), "dh": nans((Bn, H)), "s1": nans((Bn, C)), "s2": nans((Bn, C))}


def run_tail_fused(c, dtn):
    o = tail_outs(c, dtn)
    args = (act(c["dout"], dtn), act(c["x"], dtn), *tail_operands(c, dtn), o["dz"], o["dse"], o["dh"], o["s1"], o["s2"],
            c["B"], c["C"], c["H"], CODE[dtn], st())
    return args, o


@pytest.mark.parametrize("C,H", list(bh.TAIL_CASES), ids=lambda v: str(v))
@pytest.mark.parametrize("dtn", ["bf16", "f32"])
def test_single_pass_tail_backward(dtn, C, H):
    """ka_tail_bwd_fused: pre-loaded and rolled FC loops, the bf16 <11, 512> form at C = 512; the fp32 run that sets the bound
    takes the kernel's documented algebra (sums centred on the BatchNorm mean) for dse / s1 / s2"""
    named = bh.TAIL_CASES[(C, H)].get(dtn)
    f = form_is(2, C, H, dtn)
    assert bool(_lib.query("ka_tail_bwd_fused_supported", C, H, CODE[dtn])) == (named is not None) == (f is not None)
    c = bh.act_case(C, dtn, H)
    args, o = run_tail_fused(c, dtn)
    if named is None:
        fails_and_writes_nothing("ka_tail_bwd_fused", args, o.values())
        return
    assert f[1:4] == named
    _lib.call("ka_tail_bwd_fused", *args)
    torch.cuda.synchronize()
    hold("tail_fused", f"C={C} H={H} {dtn}", bh.fam_tail_fused, c, o, act_names=("dz",), alg=True)


def boundary_variants(c, dtn):
    """(label, dxc, dout_up, out_up, du_up, use_dxc, up) of the three ways a boundary launch is called"""
    dxc, dup, oup, du = act(c["dxc"], dtn), act(c["dout_up"], dtn), act(c["out_up"], dtn), act(c["du_up"], dtn)
    return (("chain", dxc, dup, oup, du, True), ("no dxc", None, dup, oup, du, True), ("heads", dxc, None, None, None, False))


BOUNDARY = [(C, H, dtn, p4) for (C, H), d in bh.TAIL_CASES.items() for dtn in d if bh.block_dx_tail_supported(C, H, dtn)
            for p4 in ((1, 0) if (C, dtn) == (256, "bf16") else (1,))]


@pytest.mark.parametrize("C,H,dtn,p4", BOUNDARY, ids=lambda v: str(v))
def test_block_boundary_launches(ka_env, C, H, dtn, p4):
    """ka_block_dx_tail_bwd, _du and _du_gate: dxc present and NULL, the heads form, batched (H % 4 == 0 with both operands) and
    un-batched loops, KA_TAIL_GATE_P4 = 0 and 1 at bf16 C = 256.  dx / du against the block-input gradient's reference, the tail
    against its reference on the launch's own stored dx / du; the three entry points keep their bit-for-bit relations"""
    ka_env.set("KA_TAIL_GATE_P4", str(p4))
    assert _lib.query("ka_block_dx_tail_bwd_supported", C, H, CODE[dtn]) == 1
    f3, f4 = form_is(3, C, H, dtn), form_is(4, C, H, dtn, p4=bool(p4))
    assert f3[1:4] == bh.TAIL_CASES[(C, H)][dtn]
    assert f4[4] == (H % 4 == 0) and f4[5] == ((C, dtn, p4) == (256, "bf16", 1))
    c = bh.act_case(C, dtn, H)
    Bn, ops = c["B"], tail_operands(c, dtn)
    x, xpool, dpool = act(c["x"], dtn), vec(c["xpool"]), vec(c["dpool"])
    tail_ref = lambda dk: (lambda cc, dt, mutant=None, alg=False: bh.fam_tail_fused(cc, dt, alg=alg, dout=back(dk)))
    for label, dxc, dup, oup, du_up, has_up in boundary_variants(c, dtn):
        case = f"C={C} H={H} {dtn} p4={p4} {label}"
        use_dxc = dxc is not None
        # the plain boundary launch
        o, dx = tail_outs(c, dtn), nans((Bn, 81, C), DT[dtn])
        _lib.call("ka_block_dx_tail_bwd", dxc, dup, oup, x, xpool, dpool, dx, *ops, o["dz"], o["dse"], o["dh"], o["s1"], o["s2"],
                  Bn, C, H, CODE[dtn], st())
        torch.cuda.synchronize()
        hold("block_dx_tail_bwd", case, bh.fam_block_dx(use_dxc, "masked" if has_up else "none"), c, {"dx": dx}, act_names=("dx",))
        hold("block_dx_tail_bwd tail", case, tail_ref(dx), c, o, act_names=("dz",), alg=True)
        # the chain form
        o2, du = tail_outs(c, dtn), nans((Bn, 81, C), DT[dtn])
        _lib.call("ka_block_dx_tail_bwd_du", dxc, du_up, x, xpool, dpool, du, *ops, o2["dz"], o2["dse"], o2["dh"], o2["s1"], o2["s2"],
                  Bn, C, H, CODE[dtn], st())
        torch.cuda.synchronize()
        du_fn = lambda cc, dt, mutant=None, alg=False: {"du": bh.ref_block_dx(cc, dt, use_dxc, "du" if has_up else "none")["du"]}
        hold("block_dx_tail_bwd_du", case, du_fn, c, {"du": du}, act_names=("du",))
        hold("block_dx_tail_bwd_du tail", case, tail_ref(du), c, o2, act_names=("dz",), alg=True)
        assert torch.equal(du, torch.where(x > 0, dx, torch.zeros_like(dx)))
        # the masked gradient of the block above is a rounded copy, so the chain reproduces the plain launch bit for bit
        for k in o:
            assert torch.equal(o[k], o2[k]), (case, k)
        # the gate form: no dz, gate / add instead
        o3, du3, gate, add = tail_outs(c, dtn), nans((Bn, 81, C), DT[dtn]), nans((Bn, C)), nans((Bn, C))
        _lib.call("ka_block_dx_tail_bwd_du_gate", dxc, du_up, x, xpool, dpool, du3, *ops, gate, add, o3["dse"], o3["dh"], o3["s1"],
                  o3["s2"], Bn, C, H, CODE[dtn], st())
        torch.cuda.synchronize()
        assert bool(torch.isnan(o3["dz"].float()).all())
        hold("block_dx_tail_bwd_du_gate", case, du_fn, c, {"du": du3}, act_names=("du",))
        dz3 = torch.addcmul(add.double()[:, None, :], du3.double(), gate.double()[:, None, :]).float().to(DT[dtn])   # fmaf, rounded once
        got = {"dz": dz3, "gate": gate, "add": add, "dse": o3["dse"], "dh": o3["dh"], "s1": o3["s1"], "s2": o3["s2"]}
        hold("block_dx_tail_bwd_du_gate tail", case, tail_ref(du3), c, got, act_names=("dz",), alg=True)
        assert torch.equal(du3, du), case
        if not f4[5]:                              # (the half-width pieces split the squares differently: their sums are equal to rounding)
            assert torch.equal(dz3, o2["dz"]), case
            for k in ("dse", "dh", "s1", "s2"):
                assert torch.equal(o3[k], o2[k]), (case, k)


GRID_H = (1, 2, 4, 8, 16, 32, 64)


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
def test_supported_implies_it_launches(dtn):
    """C = 8..512 step 8, H in 1..64, B = 1: where a `supported` query says 1 the call succeeds and meets the oracle, where it
    says 0 the call fails and writes nothing (so the LDS check inside the launcher never disagrees with the queries).
    The launch computes board 0 of a three-board case.  e32 is a maximum over the elements of a tensor, and dh of one board
    at H = 1 is ONE element: a single draw of the fp32 run's error is below a third of its typical size one time in four, and
    the correct kernel then misses MARGIN x e32 (measured: dh at f32 C = 128, H = 1 at 1.49 of it).  So e32 is taken as the
    larger of the launched board's and the whole case's: the same formulas on the same kind of data, three boards of samples."""
    n_ok = 0
    for C in range(8, 513, 8):
        for H in GRID_H:
            c3 = bh.act_case.__wrapped__(C, dtn, H)              # (not kept: 900 cases)
            c = bh.first_board(c3)
            case = f"grid C={C} H={H} {dtn}"
            ok2, ok3, oks = (bool(_lib.query(qn, C, H, CODE[dtn])) for qn in
                             ("ka_tail_bwd_fused_supported", "ka_block_dx_tail_bwd_supported", "ka_block_tail_fwd_se_supported"))
            assert (ok2, ok3, oks) == (bh.tail_fused_supported(C, H, dtn), bh.block_dx_tail_supported(C, H, dtn), bh.fwd_se_supported(C, H, dtn))
            args, o = run_tail_fused(c, dtn)
            if ok2:
                _lib.call("ka_tail_bwd_fused", *args)
                torch.cuda.synchronize()
                hold("grid tail_fused", case, bh.fam_tail_fused, c, o, act_names=("dz",), alg=True, bound=(bh.fam_tail_fused, c3))
            else:
                fails_and_writes_nothing("ka_tail_bwd_fused", args, o.values())
            o, dx = tail_outs(c, dtn), nans((1, 81, C), DT[dtn])
            args = (act(c["dxc"], dtn), act(c["dout_up"], dtn), act(c["out_up"], dtn), act(c["x"], dtn), vec(c["xpool"]), vec(c["dpool"]),
                    dx, *tail_operands(c, dtn), o["dz"], o["dse"], o["dh"], o["s1"], o["s2"], 1, C, H, CODE[dtn], st())
            if ok3:
                _lib.call("ka_block_dx_tail_bwd", *args)
                torch.cuda.synchronize()
                hold("grid block_dx_tail_bwd", case, bh.fam_block_dx(True, "masked"), c, {"dx": dx}, act_names=("dx",),
                     bound=(bh.fam_block_dx(True, "masked"), c3))
                hold("grid block_dx_tail_bwd tail", case, lambda cc, dt, mutant=None, alg=False: bh.fam_tail_fused(cc, dt, alg=alg, dout=back(dx)),
                     c, o, act_names=("dz",), alg=True, bound=(bh.fam_tail_fused, c3))
            else:
                fails_and_writes_nothing("ka_block_dx_tail_bwd", args, (dx, *o.values()))
            out, pool, sqz, se1, se = nans((1, 81, C), DT[dtn]), nans((1, 4 * C)), nans((1, C)), nans((1, H)), nans((1, 2 * C))
            args = (act(c["y"], dtn), vec(c["scale"]), vec(c["shift"]), vec(c["bsum"]), vec(c["W1"]), vec(c["b1"]), vec(c["W2"]), vec(c["b2"]),
                    act(c["res"], dtn), out, pool, sqz, se1, se, 1, C, H, CODE[dtn], st())
            if oks:
                _lib.call("ka_block_tail_fwd_se", *args)
                torch.cuda.synchronize()
                hold("grid tail_fwd_se", case, bh.fam_se_chain(True), c, {"sqz": sqz, "se1": se1, "se": se}, bound=(bh.fam_se_chain(True), c3))
                hold("grid tail_fwd_se", case, lambda cc, dt, mutant=None, alg=False: {"out": bh.ref_tail_fwd(cc, dt, se=back(se))}, c,
                     {"out": out}, act_names=("out",))
            else:
                fails_and_writes_nothing("ka_block_tail_fwd_se", args, (out, pool, sqz, se1, se))
            n_ok += ok2 + ok3 + oks
    assert n_ok > 60


@pytest.mark.parametrize("C,dtn", bh.act_cases(bh.RELU_BN_C), ids=lambda v: str(v))
def test_relu_bn_backward_and_bn_apply(C, dtn):
    """ka_relu_bn_bwd_reduce (the one kernel that recomputes its mask: exact zeros placed, every other argument a margin away
    from zero) and ka_bn_bwd_apply"""
    c = bh.relu_case(C, dtn)
    Bn = c["B"]
    da, s1, s2, dy = nans((Bn, 81, C), DT[dtn]), nans((Bn, C)), nans((Bn, C)), nans((Bn, 81, C), DT[dtn])
    _lib.call("ka_relu_bn_bwd_reduce", act(c["dh"], dtn), act(c["y"], dtn), vec(c["scale"]), vec(c["shift"]), vec(c["mean"]),
              vec(c["invstd"]), da, s1, s2, Bn, C, CODE[dtn], st())
    _lib.call("ka_bn_bwd_apply", act(c["dz"], dtn), act(c["y"], dtn), vec(c["k"]), dy, Bn, C, CODE[dtn], st())
    torch.cuda.synchronize()
    hold("relu_bn_bwd", f"C={C} {dtn}", bh.fam_relu_bn, c, {"da": da, "s1": s1, "s2": s2}, act_names=("da",))
    assert bool((da[:, [0, 40, 80], c["cz"]] == 0).all())
    hold("bn_bwd_apply", f"C={C} {dtn}", bh.fam_bn_apply, c, {"dy": dy}, act_names=("dy",))


# ------------------------------------------------------------------------------------------------ reducers and coefficients

ROWS = [(r, r) for r in (1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6147)] + [(515, 129), (4097, 3), (3, 4097)]
EPS32, MOM32 = float(torch.tensor(1e-5)), float(torch.tensor(0.1))


def ints(shape, g):
    return torch.randint(-8, 9, shape, generator=g).float()


def coeff_inputs(C, g):
    return ((torch.rand(C, generator=g) + 0.5), torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5)


def hold_coeffs(case, got, ref64, ref32, one_ulp):
    """outputs that are one rounding of a float64 value: 1 float32 ulp; those formed by further fp32 steps: MARGIN x e32"""
    for k, v in got.items():
        if k in one_ulp:
            r = bh.ulps32(back(v), ref64[k])
        else:
            r = bh.ratio(back(v), ref64[k].double(), bh.e32_of(ref32[k].double(), ref64[k].double()))
        if r >= WORST.get(("coefficients", k), (-1.0, None))[0]:
            WORST[("coefficients", k)] = (r, case)
        assert r <= 1.0, (case, k, r)


@pytest.mark.parametrize("C", [32, 96, 256])
def test_reducers_equal_exact_integer_sums(C):
    """ka_bn_reduce, ka_pair_reduce, ka_sync_reduce, ka_bn_reduce_coeffs, ka_pair_reduce_bwd_coeffs on integers in -8..8 (every
    fp64 sum exact in any order) at the row counts that reach each loop edge of colsum2_stage1_body: sums equal int64 sums to
    the bit, the count slot and the local copy are written, the one-launch forms equal the two-launch forms to the bit and the
    coefficients meet the float64 formula"""
    g = torch.Generator().manual_seed(C)
    ws = lambda: torch.empty(_lib.query("ka_reduce_workspace_doubles", C), dtype=F64, device=DEV)
    gamma, beta, rm, rv = coeff_inputs(C, g)
    mu, istd = 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    counters = torch.zeros((C + 63) // 64, dtype=torch.int32, device=DEV)
    for ra, rb in ROWS:
        a, b = ints((ra, C), g), ints((rb, C), g)
        exact = torch.cat([a.long().sum(0), b.long().sum(0)]).double()
        ad, bd = a.to(DEV), b.to(DEV)
        sums = nans((2 * C,), F64)
        _lib.call("ka_bn_reduce", ad, ra, bd, rb, C, sums, ws(), st())
        assert torch.equal(sums.cpu(), exact), ("bn_reduce", ra, rb)
        count = float(ra * 81)
        sync, local = nans((2 * C + 1,), F64), nans((2 * C + 1,), F64)
        _lib.call("ka_sync_reduce", ad, ra, bd, rb, C, count, sync, local, ws(), st())
        assert torch.equal(sync.cpu(), torch.cat([exact, torch.tensor([count], dtype=F64)])) and torch.equal(local, sync), ("sync_reduce", ra, rb)
        sync2 = nans((2 * C + 1,), F64)
        _lib.call("ka_sync_reduce", ad, ra, bd, rb, C, count, sync2, None, ws(), st())
        assert torch.equal(sync2, sync)
        # forward coefficients: one launch == reduce + coefficients from the partials, and both meet the formula
        outs = []
        for one in (True, False):
            o = {k: nans((C,)) for k in ("scale", "shift", "mean", "invstd")}
            o["running_mean"], o["running_var"] = rm.to(DEV), rv.to(DEV)
            nbt, part = torch.zeros((), dtype=torch.int64, device=DEV), ws()
            tail = (gamma.to(DEV), beta.to(DEV), o["running_mean"], o["running_var"], nbt, 0.1, 1e-5, o["scale"], o["shift"], o["mean"], o["invstd"])
            if one:
                _lib.call("ka_bn_reduce_coeffs", ad, ra, bd, rb, C, part, counters, count, *tail, st())
            else:
                _lib.call("ka_bn_reduce", ad, ra, bd, rb, C, None, part, st())
                _lib.call("ka_bn_coeffs_parts", part, count, *tail, C, st())
            torch.cuda.synchronize()
            assert int(nbt) == 1 and int(counters.abs().sum()) == 0
            outs.append(o)
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), ("bn_reduce_coeffs", k, ra, rb)
        refs = [bh.ref_bn_coeffs(exact.to(dt), count, gamma.double(), beta.double(), rm.double(), rv.double(), MOM32, EPS32, dt) for dt in (F64, F32)]
        hold_coeffs(f"fwd C={C} rows={ra},{rb}", outs[0], refs[0], refs[1], ("mean", "invstd"))
        if ra != rb:
            continue
        sums = nans((2 * C,), F64)
        _lib.call("ka_pair_reduce", ad, bd, ra, C, sums, ws(), st())
        assert torch.equal(sums.cpu(), exact), ("pair_reduce", ra)
        for train in (1, 0):
            outs = []
            for one in (True, False):
                o = {"dgamma": nans((C,)), "dbeta": nans((C,)), "k": nans((3 * C,))}
                part = ws()
                tail = (gamma.to(DEV), mu.to(DEV), istd.to(DEV), o["dgamma"], o["dbeta"], o["k"])
                if one:
                    _lib.call("ka_pair_reduce_bwd_coeffs", ad, bd, ra, C, part, counters, count, *tail, train, st())
                else:
                    _lib.call("ka_pair_reduce", ad, bd, ra, C, None, part, st())
                    _lib.call("ka_bn_bwd_coeffs_parts", part, count, *tail, C, train, st())
                torch.cuda.synchronize()
                outs.append(o)
            for k in outs[0]:
                assert torch.equal(outs[0][k], outs[1][k]), ("pair_reduce_bwd_coeffs", k, ra)
            ref = bh.ref_bn_bwd_coeffs(exact, exact, count, gamma.double(), mu.double(), istd.double(), train, F64)
            hold_coeffs(f"bwd C={C} rows={ra} train={train}", outs[0], ref, ref, ("dgamma", "dbeta", "k"))
            if not train:
                assert bool((outs[0]["k"][C:] == 0).all())


def test_bn_coefficient_arguments():
    """ka_bn_coeffs: count_dev overrides count, count = 1 keeps the biased variance, a slightly negative E[x^2] - mean^2 is
    clamped, running_mean NULL, num_batches_tracked advances once per launch; ka_bn_bwd_coeffs: train = 0, global sums that
    differ from the local ones; ka_bn_eval_coeffs_multi == three ka_bn_eval_coeffs calls; ka_affine_rows"""
    C = 96
    g = torch.Generator().manual_seed(17)
    gamma, beta, rm, rv = coeff_inputs(C, g)
    n = 5 * 81
    x = ints((n, C), g).double() / 4
    sums = torch.cat([x.sum(0), (x * x).sum(0)])
    sums[C + 3] = sums[3] ** 2 / n * (1 - 2.0 ** -40)              # E[x^2] - mean^2 slightly negative: clamped
    sums[C + 4] = sums[4] ** 2 / n                                  # and exactly zero
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)

    def run(count, count_dev, with_running=True):
        o = {k: nans((C,)) for k in ("scale", "shift", "mean", "invstd")}
        if with_running:
            o["running_mean"], o["running_var"] = rm.to(DEV), rv.to(DEV)
        _lib.call("ka_bn_coeffs", sums.to(DEV), count, count_dev, gamma.to(DEV), beta.to(DEV), o.get("running_mean"), o.get("running_var"),
                  nbt, 0.1, 1e-5, o["scale"], o["shift"], o["mean"], o["invstd"], C, st())
        torch.cuda.synchronize()
        return o

    def refs(count, with_running=True, mutant=None):
        r = (rm.double(), rv.double()) if with_running else (None, None)
        return [bh.ref_bn_coeffs(sums.to(dt), count, gamma.double(), beta.double(), *r, MOM32, EPS32, dt, mutant=mutant) for dt in (F64, F32)]

    o = run(float(n), None)
    hold_coeffs("bn_coeffs", o, *refs(float(n)), ("mean", "invstd"))
    assert float(o["invstd"][3]) == float(o["invstd"][4]) == float(torch.tensor(1.0 / math.sqrt(EPS32)))
    bad = refs(float(n), mutant="rv_biased")[0]["running_var"]
    assert bh.ratio(bad.float(), refs(float(n))[0]["running_var"], bh.e32_of(refs(float(n))[1]["running_var"].double(), refs(float(n))[0]["running_var"])) > 1
    o = run(7.0, torch.tensor([float(n)], dtype=F64, device=DEV))                      # count_dev wins
    hold_coeffs("bn_coeffs count_dev", o, *refs(float(n)), ("mean", "invstd"))
    s1 = sums.clone()
    o = run(1.0, None)                                                                  # count 1: no n / (n - 1)
    hold_coeffs("bn_coeffs count=1", o, *refs(1.0), ("mean", "invstd"))
    o = run(float(n), None, with_running=False)
    hold_coeffs("bn_coeffs no running stats", o, *refs(float(n), False), ("mean", "invstd"))
    assert int(nbt) == 4 and torch.equal(s1, sums)
    # backward coefficients
    mu, istd = 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    loc, glo = ints((2 * C,), g).double() * 3, ints((2 * C,), g).double() * 5
    for train in (1, 0):
        for cd in (None, torch.tensor([float(n)], dtype=F64, device=DEV)):
            o = {"dgamma": nans((C,)), "dbeta": nans((C,)), "k": nans((3 * C,))}
            _lib.call("ka_bn_bwd_coeffs", loc.to(DEV), glo.to(DEV), float(n) if cd is None else 3.0, cd, gamma.to(DEV), mu.to(DEV), istd.to(DEV),
                      o["dgamma"], o["dbeta"], o["k"], C, train, st())
            torch.cuda.synchronize()
            ref = bh.ref_bn_bwd_coeffs(loc, glo, float(n), gamma.double(), mu.double(), istd.double(), train, F64)
            hold_coeffs(f"bn_bwd_coeffs train={train}", o, ref, ref, ("dgamma", "dbeta", "k"))
            if not train:
                assert bool((o["k"][C:] == 0).all())
                assert bh.ulps32(bh.ref_bn_bwd_coeffs(loc, glo, float(n), gamma.double(), mu.double(), istd.double(), 0, F64, mutant="eval_k")["k"], ref["k"]) > 1
    # eval coefficients: three layers of different C in one launch == three launches, and the float64 formula
    layers, rows = [], []
    for Cl in (6, 96, 256):
        p = [t.to(DEV) for t in coeff_inputs(Cl, g)]
        single, multi = (nans((Cl,)), nans((Cl,))), (nans((Cl,)), nans((Cl,)))
        _lib.call("ka_bn_eval_coeffs", *p, 1e-5, *single, Cl, st())
        rows.append([t.data_ptr() for t in (*p, *multi)] + [Cl, int(torch.tensor(1e-5).view(torch.int32))])
        layers.append((p, single, multi))
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    _lib.call("ka_bn_eval_coeffs_multi", table, 3, 256, st())
    torch.cuda.synchronize()
    for p, single, multi in layers:
        assert torch.equal(single[0], multi[0]) and torch.equal(single[1], multi[1])
        rr = [bh.ref_bn_eval_coeffs(*(t.cpu().double() for t in p), EPS32, dt) for dt in (F64, F32)]
        hold_coeffs("bn_eval_coeffs", {"scale": multi[0], "shift": multi[1]}, rr[0], rr[1], ())
    # ka_affine_rows
    xin, a, s = torch.randn(7, C, generator=g), torch.rand(C, generator=g), torch.randn(C, generator=g)
    out = nans((7, C))
    _lib.call("ka_affine_rows", xin.to(DEV), a.to(DEV), s.to(DEV), 1.0 / 81.0, out, 7, C, st())
    mul = float(torch.tensor(1.0 / 81.0))
    r64, r32 = (bh.ref_affine_rows(xin, a, s, mul, dt) for dt in (F64, F32))
    assert bh.ratio(out, r64, bh.e32_of(r32.double(), r64)) <= 1.0


# ------------------------------------------------------------------------------------------------ layout kernels


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
def test_layout_kernels_are_exact(dtn):
    g = torch.Generator().manual_seed(29)
    for cobs, cpad in ((50, 64), (46, 96)):
        obs = torch.randn(6, cobs, 9, 9, generator=g)
        for idx in (None, torch.tensor([5, 5, 0, 3, 1, 3, 2])):
            nb = 6 if idx is None else idx.numel()
            out = nans((nb, 81, cpad), DT[dtn])
            _lib.call("ka_obs_to_nhwc", obs.to(DEV), None if idx is None else idx.to(DEV), out, nb, cobs, cpad, CODE[dtn], st())
            assert torch.equal(out.cpu(), bh.ref_obs_to_nhwc(obs, idx, cpad).to(DT[dtn])), (cobs, cpad, idx is None)
    for C in (6, 96, 256):
        x = torch.randn(3, 81, C, generator=g).to(DT[dtn])
        out = nans((3, C, 9, 9))
        _lib.call("ka_nhwc_to_nchw", x.to(DEV), out, 3, C, CODE[dtn], st())
        assert torch.equal(out.cpu(), bh.ref_nhwc_to_nchw(x.float())), C


# ------------------------------------------------------------------------------------------------ guard rows


@pytest.mark.parametrize("C,H,dtn", [(32, 4, "bf16"), (16, 4, "f32"), (6, 0, "bf16"), (6, 0, "f32"), (64, 4, "bf16"), (256, 16, "bf16")],
                         ids=lambda v: str(v))
def test_guard_rows_stay_intact(C, H, dtn):
    """One guarded run per entry point of the activation kernels at B = 3: the smallest 16-byte form, the smallest pair form, a
    shape with the SE chain inside and the half-width batched gate form.  Output guards intact, results identical with zero
    and with NaN input guards: the clamped loads of the batched loops stay inside the board"""
    c = bh.act_case(C, dtn, H)
    Bn, dt, code = c["B"], DT[dtn], CODE[dtn]
    A = lambda k: act(c[k], dtn)
    v = {k: vec(c[k]) for k in ("scale", "shift", "mean", "invstd")}
    actshape, f = ((Bn, 81, C), dt), lambda *s: ((Bn, *s), torch.float32)
    check_guarded(lambda b: _lib.call("ka_block_tail_fwd", b["y"], v["scale"], v["shift"], b["se"], b["res"], b["out"], b["pool"], Bn, C, code, st()),
                  {"y": A("y"), "se": vec(c["se"]), "res": A("res")}, {"out": actshape, "pool": f(4 * C)})
    check_guarded(lambda b: _lib.call("ka_pool_fwd", b["x"], b["pool"], Bn, C, code, st()), {"x": A("x")}, {"pool": f(4 * C)})
    check_guarded(lambda b: _lib.call("ka_block_dx", b["dxc"], b["dup"], b["oup"], b["x"], b["xpool"], b["dpool"], b["dx"], Bn, C, code, st()),
                  {"dxc": A("dxc"), "dup": A("dout_up"), "oup": A("out_up"), "x": A("x"), "xpool": vec(c["xpool"]), "dpool": vec(c["dpool"])},
                  {"dx": actshape})
    check_guarded(lambda b: _lib.call("ka_tail_bwd_reduce", b["dout"], b["out"], b["y"], v["scale"], v["shift"], b["se"], b["dse"], Bn, C, code, st()),
                  {"dout": A("dout"), "out": A("x"), "y": A("y"), "se": vec(c["se_bwd"])}, {"dse": f(2 * C)})
    check_guarded(lambda b: _lib.call("ka_tail_bwd_dz", b["dout"], b["out"], b["y"], b["se"], b["dsq"], v["mean"], v["invstd"], b["dz"], b["s1"],
                                      b["s2"], Bn, C, code, st()),
                  {"dout": A("dout"), "out": A("x"), "y": A("y"), "se": vec(c["se_bwd"]), "dsq": vec(c["dsq"])},
                  {"dz": actshape, "s1": f(C), "s2": f(C)})
    check_guarded(lambda b: _lib.call("ka_relu_bn_bwd_reduce", b["dh"], b["y"], v["scale"], v["shift"], v["mean"], v["invstd"], b["da"], b["s1"],
                                      b["s2"], Bn, C, code, st()),
                  {"dh": A("dout"), "y": A("y")}, {"da": actshape, "s1": f(C), "s2": f(C)})
    kk = torch.cat([v["scale"], v["shift"], v["mean"]])
    check_guarded(lambda b: _lib.call("ka_bn_bwd_apply", b["dz"], b["y"], kk, b["dy"], Bn, C, code, st()), {"dz": A("dout"), "y": A("y")},
                  {"dy": actshape})
    if not H:
        return
    W1, W2, b1, b2 = vec(c["W1"]), vec(c["W2"]), vec(c["b1"]), vec(c["b2"])
    if bh.fwd_se_supported(C, H, dtn):
        check_guarded(lambda b: _lib.call("ka_block_tail_fwd_se", b["y"], v["scale"], v["shift"], b["bsum"], W1, b1, W2, b2, b["res"], b["out"],
                                          b["pool"], b["sqz"], b["se1"], b["se"], Bn, C, H, code, st()),
                      {"y": A("y"), "bsum": vec(c["bsum"]), "res": A("res")},
                      {"out": actshape, "pool": f(4 * C), "sqz": f(C), "se1": f(H), "se": f(2 * C)})
    tin = {"out": A("x"), "y": A("y"), "se": vec(c["se_bwd"]), "se1": vec(c["se1"])}
    tout = {"dz": actshape, "dse": f(2 * C), "dh": f(H), "s1": f(C), "s2": f(C)}
    mid = lambda b: (b["y"], v["scale"], v["shift"], b["se"], b["se1"], W2, W1, v["mean"], v["invstd"])
    check_guarded(lambda b: _lib.call("ka_tail_bwd_fused", b["dout"], b["out"], *mid(b), b["dz"], b["dse"], b["dh"], b["s1"], b["s2"], Bn, C, H, code, st()),
                  dict(tin, dout=A("dout")), tout)
    if not bh.block_dx_tail_supported(C, H, dtn):
        return
    din = dict(tin, dxc=A("dxc"), dup=A("dout_up"), oup=A("out_up"), du_up=A("du_up"), xpool=vec(c["xpool"]), dpool=vec(c["dpool"]))
    check_guarded(lambda b: _lib.call("ka_block_dx_tail_bwd", b["dxc"], b["dup"], b["oup"], b["out"], b["xpool"], b["dpool"], b["dx"], *mid(b),
                                      b["dz"], b["dse"], b["dh"], b["s1"], b["s2"], Bn, C, H, code, st()), din, dict(tout, dx=actshape))
    check_guarded(lambda b: _lib.call("ka_block_dx_tail_bwd_du", b["dxc"], b["du_up"], b["out"], b["xpool"], b["dpool"], b["dx"], *mid(b),
                                      b["dz"], b["dse"], b["dh"], b["s1"], b["s2"], Bn, C, H, code, st()), din, dict(tout, dx=actshape))
    gout = {k: s for k, s in tout.items() if k != "dz"}
    check_guarded(lambda b: _lib.call("ka_block_dx_tail_bwd_du_gate", b["dxc"], b["du_up"], b["out"], b["xpool"], b["dpool"], b["dx"], *mid(b),
                                      b["gate"], b["add"], b["dse"], b["dh"], b["s1"], b["s2"], Bn, C, H, code, st()),
                  din, dict(gout, dx=actshape, gate=f(C), add=f(C)))
