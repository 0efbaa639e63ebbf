"""CPU side of the board-kernel oracle (tests/board_helpers.py): the float64 references equal torch autograd through the
model's formulas on the edge data, every mutant lies outside the bound the kernels are held to (judged as a kernel would
be: rounded to the storage dtype first), the case lists cover every form, and the launch-form mirror agrees with the
library's own queries (which launch nothing, so they run here)."""
import pytest
import torch
import torch.nn.functional as F

import board_helpers as bh
from board_helpers import F32, F64
from oracle import keisei_oracle as orc

ATOL = 2.0 ** -52 * 81 * 512       # float64 against float64: one ulp per term of the longest sum (2 C = 512 products over 81 squares)


def nchw(t):
    return t.permute(0, 2, 1).reshape(t.shape[0], t.shape[2], 9, 9)


def same(a, b, what):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= ATOL * max(1.0, float(b.abs().max())), what


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
def test_tail_references_equal_autograd(dtn):
    """forward tail, SE chain and the whole backward tail against autograd through relu(bn(y) sigmoid(a) + b + x) with the
    SE linears in the graph (the chain's own se1 carries exact zeros: ReLU outputs)"""
    C, H = 16, 4
    c = dict(bh.act_case(C, dtn, H))
    yhat = (c["y"] - c["mean"]) * c["invstd"]
    gam = (c["scale"] / c["invstd"]).expand(bh.B, C).clone().requires_grad_(True)          # per board: s1 / s2 are per-board partials
    bet = (c["shift"] + c["mean"] * c["scale"]).expand(bh.B, C).clone().requires_grad_(True)
    z = yhat * gam[:, None] + bet[:, None]
    sqz = z.mean(1)
    hpre = sqz @ c["W1"].t() + c["b1"]
    h = torch.relu(hpre)
    se = h @ c["W2"].t() + c["b2"]
    v = z * torch.sigmoid(se[:, None, :C]) + se[:, None, C:] + c["res"]
    out = torch.relu(v)
    gv, gz, gse, ghpre, gsqz, gg, gb = torch.autograd.grad((out * c["dout"]).sum(), [v, z, se, hpre, sqz, gam, bet])
    # forward references on the same operands
    c["bsum"] = c["y"].sum(1)
    ch = bh.ref_se_chain(c, F64)
    same(ch["sqz"], sqz.detach(), "sqz"); same(ch["se1"], h.detach(), "se1"); same(ch["se"], se.detach(), "se")
    same(bh.ref_tail_fwd(c, F64, se=se.detach()), out.detach(), "out")
    c["se_bwd"], c["se1"] = se.detach(), h.detach()
    for alg in (False, True):                      # the fused tail's documented algebra is the same function
        r = bh.ref_tail_bwd(c, F64, out=out.detach(), fused_algebra=alg)
        for k, ref in (("du", gv), ("dz", gz), ("dse", gse), ("dh", ghpre), ("dsq", gsqz), ("s1", gb), ("s2", gg)):
            same(r[k], ref, f"{k} alg={alg}")
    r = bh.ref_tail_bwd(c, F64, out=out.detach(), dsq=gsqz)
    same(r["dz"], gz, "dz from a given dsq")


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
@pytest.mark.parametrize("C", [6, 32])
def test_pool_and_block_dx_references_equal_autograd(dtn, C):
    """pool = orc.global_pool + the tie count; dx = autograd through it on the edge planes: ties share, std == 0 gives 0"""
    c = dict(bh.act_case(C, dtn))
    x = c["x"].clone().requires_grad_(True)
    pool = orc.global_pool(nchw(x))
    p = bh.ref_pool(c["x"], F64)
    same(p[:, :3 * C], pool.detach(), "pool")
    for kind, (b, ch) in c["slots"].items():
        assert float(p[b, 3 * C + ch]) == bh.EDGE_TIES[kind], kind
        if kind in ("zero", "const"):
            assert float(p[b, 2 * C + ch]) == 0.0
    c["xpool"] = p                                 # (the case carries it rounded to float32, as the kernel reads it)
    gx = torch.autograd.grad((pool * c["dpool"]).sum(), x)[0]
    assert bool(torch.isfinite(gx).all())
    same(bh.ref_block_dx(c, F64, False, "none")["dx"], gx, "heads form")
    full = gx + c["dxc"] + c["dout_up"] * (c["out_up"] > 0)
    same(bh.ref_block_dx(c, F64, True, "masked")["dx"], full, "masked form")
    r = bh.ref_block_dx(c, F64, True, "du")
    same(r["dx"], full, "du form"); same(r["du"], full * (c["x"] > 0), "du")


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
def test_relu_bn_references_equal_autograd(dtn):
    C = 6
    c = bh.relu_case(C, dtn)
    assert bh.relu_margin_ok(c)
    yhat = (c["y"] - c["mean"]) * c["invstd"]
    gam = (c["scale"] / c["invstd"]).expand(bh.B, C).clone().requires_grad_(True)
    bet = (c["shift"] + c["mean"] * c["scale"]).expand(bh.B, C).clone().requires_grad_(True)
    # (gamma yhat + beta rebuilt from scale / shift need not be exactly 0 at the placed zeros, so the ReLU is written as its
    #  mask [scale y + shift > 0] on the operands themselves: relu'(0) = 0, as autograd has it)
    lin = yhat * gam[:, None] + bet[:, None]
    hh = lin * (c["y"] * c["scale"] + c["shift"] > 0)
    gl, gg, gb = torch.autograd.grad((hh * c["dh"]).sum(), [lin, gam, bet])
    r = bh.ref_relu_bn_bwd(c, F64)
    same(r["da"], gl, "da"); same(r["s1"], gb, "s1"); same(r["s2"], gg, "s2")
    assert bool((r["da"][:, [0, 40, 80], c["cz"]] == 0).all())


def test_bn_coefficient_references_equal_batch_norm():
    g = torch.Generator().manual_seed(5)
    N, C, eps, mom = 7, 5, 1e-5, 0.1
    x = torch.randint(-8, 9, (N, C, 9, 9), generator=g).double().requires_grad_(True)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).double().requires_grad_(True), torch.randn(C, generator=g).double().requires_grad_(True)
    rm, rv = torch.randn(C, generator=g).double(), (torch.rand(C, generator=g) + 0.5).double()
    dz = torch.randn(N, C, 9, 9, generator=g).double()
    sums = torch.cat([x.detach().sum((0, 2, 3)), (x.detach() ** 2).sum((0, 2, 3))])
    count = float(N * 81)
    rm2, rv2 = rm.clone(), rv.clone()
    z = F.batch_norm(x, rm2, rv2, gamma, beta, training=True, momentum=mom, eps=eps)
    r = bh.ref_bn_coeffs(sums, count, gamma.detach(), beta.detach(), rm, rv, mom, eps, F64)
    same(x.detach() * r["scale"][None, :, None, None] + r["shift"][None, :, None, None], z.detach(), "train scale / shift")
    same(r["running_mean"], rm2, "running_mean"); same(r["running_var"], rv2, "running_var (unbiased)")
    one = bh.ref_bn_coeffs(sums, 1.0, gamma.detach(), beta.detach(), rm, rv, mom, eps, F64)
    same(one["running_var"], 0.9 * rv + 0.1 * (sums[C:] - sums[:C] ** 2).clamp_min(0), "count 1: biased")
    gx, gg, gb = torch.autograd.grad((z * dz).sum(), [x, gamma, beta])
    yhat = (x.detach() - r["mean"][None, :, None, None]) * r["invstd"][None, :, None, None]
    bs = torch.cat([dz.sum((0, 2, 3)), (dz * yhat).sum((0, 2, 3))])
    k = bh.ref_bn_bwd_coeffs(bs, bs, count, gamma.detach(), r["mean"], r["invstd"], 1, F64)
    same(k["dgamma"], gg, "dgamma"); same(k["dbeta"], gb, "dbeta")
    kk = k["k"].reshape(3, C)[:, None, :, None, None]
    same(kk[0] * dz + kk[1] + kk[2] * x.detach(), gx, "train dy")
    # eval mode
    ze = F.batch_norm(x, rm, rv, gamma, beta, training=False, eps=eps)
    e = bh.ref_bn_eval_coeffs(gamma.detach(), beta.detach(), rm, rv, eps, F64)
    same(x.detach() * e["scale"][None, :, None, None] + e["shift"][None, :, None, None], ze.detach(), "eval scale / shift")
    gxe = torch.autograd.grad((ze * dz).sum(), x)[0]
    ke = bh.ref_bn_bwd_coeffs(bs, bs, count, gamma.detach(), rm, 1 / torch.sqrt(rv + eps), 0, F64)["k"].reshape(3, C)
    assert bool((ke[1:] == 0).all())
    same(ke[0][None, :, None, None] * dz, gxe, "eval dy")
    # the two coefficient mutants lie outside one float32 ulp / the bound
    assert bh.ulps32(bh.ref_bn_bwd_coeffs(bs, bs, count, gamma.detach(), rm, 1 / torch.sqrt(rv + eps), 0, F64, mutant="eval_k")["k"], ke.reshape(-1)) > 1
    bad = bh.ref_bn_coeffs(sums, count, gamma.detach(), beta.detach(), rm, rv, mom, eps, F64, mutant="rv_biased")
    r32 = bh.ref_bn_coeffs(sums, count, gamma.detach(), beta.detach(), rm, rv, mom, eps, F32)
    assert bh.ratio(bad["running_var"].float(), r["running_var"], bh.e32_of(r32["running_var"].double(), r["running_var"])) > 1


def test_layout_references():
    g = torch.Generator().manual_seed(3)
    obs = torch.randn(5, 7, 9, 9, generator=g)
    idx = torch.tensor([4, 4, 0, 2])
    out = bh.ref_obs_to_nhwc(obs, idx, 16)
    assert out.shape == (4, 81, 16) and bool((out[:, :, 7:] == 0).all())
    assert float(out[1, 9 * 3 + 5, 2]) == float(obs[4, 2, 3, 5])
    assert torch.equal(bh.ref_nhwc_to_nchw(out)[:, :7], obs[idx])


FAMILY_CASES = [(name, args) for name, spec in bh.FAMILIES.items() for args in spec[3]()]


@pytest.mark.parametrize("name,args", FAMILY_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_reference_inside_and_every_mutant_outside_the_bound(name, args):
    """The float64 reference, stored as the kernel stores it, is inside its own bound; each mutant the family carries is outside
    it on this case -- with the fp32 run taking the direct formulas and, for the single-pass tail, its documented algebra."""
    fn, _, _, _, mutants = bh.FAMILIES[name]
    c = bh.family_case(name, args)
    for alg in ((False, True) if name == "tail_fused" else (False,)):
        r = bh.judge_family(name, c, bh.as_stored(name, c, fn(c, F64)), alg=alg)
        assert max(r.values()) <= 1.0, (alg, r)
        for m in mutants:
            r = bh.judge_family(name, c, bh.as_stored(name, c, fn(c, F64, mutant=m)), alg=alg)
            assert max(r.values()) > 1.0, f"mutant {m} is inside the bound (alg={alg}): {r}"


def test_mutant_lists_cover_the_axes():
    """every mutant of the issue's list is carried by a reference; every family that carries one has a case of each dtype and,
    where the family has both, of the 16-byte and of the channel-pair form; every edge plane sits in every activation case"""
    need = {"dsq81", "k2", "mask_ge", "max_not_div", "max_first", "std_nozero", "sig_not_dsig", "dh_mask", "std_corr1",
            "du_up_remask", "s2_no_addSy", "rv_biased", "eval_k", "sq80_twice", "board_row"}
    assert need <= set(bh.MUTANTS)
    carried = {}
    for name, spec in bh.FAMILIES.items():
        cases = spec[3]()
        assert {a[-1] for a in cases} == {"bf16", "f32"}, name
        for m in spec[4]:
            carried.setdefault(m, []).append(name)
        if name in ("tail_fwd", "tail_fwd_nores", "pool", "block_dx", "block_dx_heads"):
            kinds = {bh.board_form(0, a[0], 0, a[1])[0] for a in cases}
            assert kinds == {"p16", "pair"}, name
            assert any(bh.board_form(0, a[0], 0, a[1])[:4] == ("pair", 256, 41, 2) for a in cases), "two-pass pair form"
        if name == "tail_fused":
            loops = {bh.board_form(2, a[0], a[1], a[2])[3] for a in cases}
            assert loops == {"pre", "rolled"}
            assert ("p16", 512, 11) in {bh.board_form(2, a[0], a[1], a[2])[:3] for a in cases if a[2] == "bf16"}
    assert need - {"rv_biased", "eval_k"} <= set(carried)          # (those two: test_bn_coefficient_references...)
    for m, fams in bh.MUTANTS.items():
        assert fams, m
    for C, dtn in bh.act_cases():
        assert set(bh.act_case(C, dtn)["slots"]) == set(bh.EDGE_KINDS)
    assert any(bh.fwd_se_supported(C, H, dtn) and H < 4 for C, H, dtn in bh.se_cases())
    assert bh.board_form(4, 256, 16, "bf16") == ("p16", 512, 11, "pre", True, True)            # the default gate form: half-width
    assert bh.board_form(4, 256, 16, "bf16", p4=False) == ("p16", 512, 6, "pre", True, False)
    assert bh.board_form(4, 64, 2, "bf16")[4] is False                                          # H % 4 != 0: un-batched loop


@pytest.mark.parametrize("C,dtn", [(C, dtn) for dtn in ("bf16", "f32") for C in bh.RELU_BN_C])
def test_relu_margin_holds_for_the_chosen_seeds(C, dtn):
    c = bh.relu_case(C, dtn)
    assert bh.relu_margin_ok(c)
    a32 = c["y"].float() * c["scale"].float() + c["shift"].float()
    assert torch.equal(a32 > 0, (c["y"] * c["scale"] + c["shift"]) > 0)        # fp32, fused or not, takes the same side


def test_case_forms_are_the_ones_named():
    for (C, dtn, pairs), f in bh.FWD_CASES.items():
        assert bh.board_form(0, C, 0, dtn, pairs)[:len(f)] == f, (C, dtn, pairs)
    for (C, H), d in bh.TAIL_CASES.items():
        for dtn in ("bf16", "f32"):
            f = bh.board_form(2, C, H, dtn)
            assert (f is None) == (dtn not in d), (C, H, dtn)
            if f:
                assert f[1:4] == d[dtn], (C, H, dtn)
    # the <11, 256> instantiations cannot be reached: a 256-thread shape has at most 16 channel pieces, hence >= 16 slices
    for dtn in ("bf16", "f32"):
        for C in range(2, 2050, 2):
            p = bh.board16_plan(C, dtn)
            assert p is None or p[0] == 512 or p[1] <= 6


def test_form_mirror_agrees_with_the_library():
    """ka_board_form and the three `supported` queries against the Python mirror on C = 2..518, nine H, both dtypes; the LDS
    footprint tail_bwd_launch checks never exceeds its limit where a query says 1"""
    from keisei_amd import _lib
    for dtn in ("bf16", "f32"):
        code = bh.CODE[dtn]
        for C in range(2, 520, 2):
            for H in (1, 2, 3, 4, 5, 8, 16, 32, 64):
                for k in range(5):
                    assert _lib.query("ka_board_form", k, C, H, code) == bh.encode_form(bh.board_form(k, C, H, dtn)), (k, C, H, dtn)
                assert bool(_lib.query("ka_block_tail_fwd_se_supported", C, H, code)) == bh.fwd_se_supported(C, H, dtn), (C, H, dtn)
                assert bool(_lib.query("ka_tail_bwd_fused_supported", C, H, code)) == bh.tail_fused_supported(C, H, dtn), (C, H, dtn)
                assert bool(_lib.query("ka_block_dx_tail_bwd_supported", C, H, code)) == bh.block_dx_tail_supported(C, H, dtn), (C, H, dtn)
                if bh.tail_fused_supported(C, H, dtn):
                    assert bh.tail_bwd_lds_bytes(C, H, dtn, bh.block_dx_tail_supported(C, H, dtn)) <= 64 * 1024
