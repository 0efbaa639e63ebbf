"""Every form of csrc/conv3x3.hip -- conv3x3_kernel, conv3x3_pc_kernel, conv3x3_pc2_kernel and conv3x3_corner_kernel, as
conv_dispatch chooses them from B, the channels, the dtype and the KA_CONV_* switches -- held to an exact integer oracle
(tests/conv_helpers.py).  With small-integer operands every product and every fp32 partial sum is exact whatever the order, so
every output of ka_conv3x3_fwd, ka_conv3x3_fwd_keep, ka_conv3x3_dgrad_fused and ka_conv3x3_dgrad_fused_gated must equal the fp64
reference on ALL boards, element for element with no tolerance (torch.equal: NaN differs from everything, the sign of a zero is
not compared), and a single dropped or misplaced product fails with a message that says where it is.  Each call asserts through
ka_conv_route_counts that exactly the intended kernels ran; each is made on NaN-prefilled outputs and again between guard
rows.  The per-workgroup partials (sqpart, ep_s1, ep_s2) are compared as column sums over all rows, taken in fp64 here, every
row written.  One case with outputs past 256 pins round-to-nearest-even and which values the sums are taken from; one on
Gaussian data bounds the accumulation error, about which exactness says nothing.  tests/test_conv_exact_cpu.py proves the
oracle on the CPU."""
import pytest
import torch

import conv_helpers as ch
from keisei_amd import _lib
from test_hip_conv_bounds import check_guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf, f32 = torch.bfloat16, torch.float32
ACTIVATIONS = ("x", "h", "out", "a", "in2", "y", "dy", "dh", "da")     # stored in the form's dtype; everything else fp32 / fp64


def st():
    return _lib.stream_ptr()


def routes():
    out = torch.zeros(len(ch.ROUTES), dtype=torch.int64)
    _lib.call("ka_conv_route_counts", out.data_ptr(), len(ch.ROUTES))
    return out


def select(ka_env, env):
    """The form's switches set, every other switch of conv_dispatch unset."""
    env = dict(env)
    for name in ch.SWITCHES:
        if name in env:
            ka_env.set(name, env[name])
        else:
            ka_env.unset(name)


def counted(label, expected, name, *args):
    """One call of an ABI entry; each counter of `expected` must rise by one and no other may move."""
    before = routes()
    _lib.call(name, *args)
    rose = {n: int(d) for n, d in zip(ch.ROUTES, routes() - before) if d}
    assert rose == {r: 1 for r in expected}, f"{label}: expected one launch on each of {expected}, counters rose by {rose}"


_DEVICE = {}


def on_device(d, dtype):
    """A case's tensors on the device, once per (case, dtype): activations and their references in dtype, sums as they are."""
    key = (id(d), dtype)
    if key not in _DEVICE:
        conv = {}
        for name, v in d._asdict().items():
            if isinstance(v, torch.Tensor):
                conv[name] = v.to(DEV, dtype if name in ACTIVATIONS else v.dtype)
            elif isinstance(v, tuple):
                conv[name] = tuple(t.to(DEV) for t in v)
        _DEVICE[key] = (d, d._replace(**conv))               # (the host case is kept alive: its id is the key)
    return _DEVICE[key][1]


_PACKS = {}


def pack(w, dtype, mode, Nout, Kin):
    """ka_pack_conv3x3 of w (Co, Ci, 3, 3) into Nout x Kin channels, once per weight tensor."""
    key = (id(w), dtype, mode, Nout, Kin)
    if key not in _PACKS:
        cpk = 32 if dtype == bf else 16
        buf = torch.zeros(9 * (Kin // cpk) * (Nout // 16) * 1024, dtype=torch.uint8, device=DEV)
        wd = w.contiguous().to(DEV)
        _lib.call("ka_pack_conv3x3", wd, buf, w.shape[0], w.shape[1], Nout, Kin, mode, _lib.dtype_code(dtype), st())
        torch.cuda.synchronize()
        _PACKS[key] = (w, buf)
    return _PACKS[key][1]


def conv_pack(d, dtype, Cin, Cout):
    """The pack of a case: mode 0 packs w (Cout, Cin); mode 1 packs the forward layer's w (Cin, Cout) flipped and transposed."""
    adjoint = isinstance(d, ch.Dgrad) or d.adjoint
    return pack(d.w, dtype, 1 if adjoint else 0, Cout, Cin)


def nan_outputs(outs):
    return {n: torch.full(shape, float("nan"), dtype=dt, device=DEV) for n, (shape, dt) in outs.items()}


def require_equal(label, got, exp, B):
    if not torch.equal(got, exp):
        pytest.fail(ch.explain(label, got, exp, B))


def require_colsum(label, got, exp_rows, B):
    """Per-workgroup partials: every row written, the column sums over all rows (fp64, taken here) equal to the reference's."""
    assert bool(torch.isfinite(got).all()), f"{label}: a row was not written"
    sums, exp = got.double().sum(0), exp_rows.double().sum(0)
    if not torch.equal(sums, exp):
        pytest.fail(ch.explain(label + " (column sums over all rows)", sums[None], exp[None], 1))


def run_fwd(label, host, B, Cin, Cout, dtype, expected, keep=False, guard=False):
    """ka_conv3x3_fwd (keep: ka_conv3x3_fwd_keep with x_out) on the first B boards of a case: out, bsum, sqpart [, x_out] exact."""
    D = ch.take(on_device(host, dtype), B)
    wp = conv_pack(host, dtype, Cin, Cout)
    rows, code = _lib.query("ka_conv3x3_sqpart_rows", B), _lib.dtype_code(dtype)
    outs = {"out": ((B, 81, Cout), dtype), "bsum": ((B, Cout), f32), "sq": ((rows, Cout), f32)}
    if keep:
        outs["xk"] = ((B, 81, Cin), dtype)

    def call(t):
        if keep:
            counted(label, expected, "ka_conv3x3_fwd_keep", t["x"], wp, t["out"], D.scale, D.shift, t.get("bias"), int(D.relu), t["bsum"],
                    t["sq"], t["xk"], B, Cin, Cout, code, st())
        else:
            counted(label, expected, "ka_conv3x3_fwd", t["x"], wp, t["out"], D.scale, D.shift, t.get("bias"), int(D.relu), t["bsum"],
                    t["sq"], B, Cin, Cout, code, st())

    inputs = {"x": D.x}
    if D.bias is not None:
        inputs["bias"] = D.bias
    if guard:
        m = check_guarded(call, inputs, outs)
        label += " (guarded)"
    else:
        m = {**inputs, **nan_outputs(outs)}
        call(m)
    require_equal(label + ": out", m["out"], D.out, B)
    require_equal(label + ": bsum", m["bsum"], D.bsum, B)
    require_colsum(label + ": sqpart", m["sq"], D.sq, B)
    if keep:
        require_equal(label + ": x_out", m["xk"], D.h, B)
    return m


def run_dgrad(label, host, B, Cin, Cout, expected, masked, guard=False):
    """ka_conv3x3_dgrad_fused (a case with gate | add: ka_conv3x3_dgrad_fused_gated) on the first B boards: dy_out, out (masked:
    da), bsum (of the unmasked dh) and, masked, ep_s1 / ep_s2 exact."""
    D = ch.take(on_device(host, bf), B)
    wp = conv_pack(host, bf, Cin, Cout)
    rows, gated = _lib.query("ka_conv3x3_sqpart_rows", B), D.ga is not None
    k = D.k
    outs = {"out": ((B, 81, Cout), bf), "dy": ((B, 81, Cin), bf), "bsum": ((B, Cout), f32)}
    inputs = {"a": D.a, "in2": D.in2}
    if masked:
        outs.update(e1=((rows, Cout), f32), e2=((rows, Cout), f32))
        inputs["y"] = D.y
    if gated:
        inputs["ga"] = D.ga.reshape(2 * B, Cin)
    ep = D.ep if masked else (None,) * 4

    def call(t):
        tail = (t.get("y"), *ep, t.get("e1"), t.get("e2"), B, Cin, Cout, 1, st())
        if gated:
            counted(label, expected, "ka_conv3x3_dgrad_fused_gated", t["a"], t["ga"], t["in2"], k, t["dy"], wp, t["out"], t["bsum"], *tail)
        else:
            counted(label, expected, "ka_conv3x3_dgrad_fused", t["a"], t["in2"], k, t["dy"], wp, t["out"], t["bsum"], *tail)

    if guard:
        m = check_guarded(call, inputs, outs)
        label += " (guarded)"
    else:
        m = {**inputs, **nan_outputs(outs)}
        call(m)
    require_equal(label + ": dy_out", m["dy"], D.dy, B)
    require_equal(label + (": da" if masked else ": out"), m["out"], D.da if masked else D.dh, B)
    require_equal(label + ": bsum", m["bsum"], D.bsum, B)
    if masked:
        require_colsum(label + ": ep_s1", m["e1"], D.s1, B)
        require_colsum(label + ": ep_s2", m["e2"], D.s2, B)
    return m


def both(run, *args, **kw):
    """On NaN-prefilled outputs, then between guard rows."""
    run(*args, **kw)
    run(*args, guard=True, **kw)


# ------------------------------------------------------------------------------------------------ (a) the generic kernel
GENERIC = ("conv",)


def geo_ids(cases):
    return [g.id for g in cases]


@pytest.mark.parametrize("geo", ch.GEOMETRY + ch.TUNED + ch.PADDED, ids=geo_ids(ch.GEOMETRY + ch.TUNED + ch.PADDED))
def test_generic_kernel_channel_geometry(ka_env, geo):
    """(a) conv3x3_kernel at B = 1, 2, 3, 5, bf16 and fp32: every branch of the chunk choice (bf16 Cin 32, 96, 160, 192, 256 =
    chunks of 32, 32 x 3, 32 x 5, 64 x 3, 128 x 2; fp32 16, 48, 256), partial 64-wide slabs and waves without a tile (Cout 16,
    48, 80, 144, 272), KA_CONV_NTW, KA_CONV_KC, KA_CONV_WM=2 (odd B: the last workgroup's second board is missing) and padded
    packs (Co < Nout; Ci < Kin with data in the padded input channels, which must meet zero weights).  The forward pack, the
    mode-1 data-gradient pack through the same entry and, bf16, ka_conv3x3_dgrad_fused with the plain and the masked epilogue."""
    select(ka_env, geo.env)
    name, dt = f"conv3x3_kernel {geo.id}", geo.dtype
    fwd, adj = ch.geo_fwd(geo), ch.geo_fwd(geo, adjoint=True)
    two = ch.geo_dgrad(geo) if dt == bf and not (geo.Cin_real or geo.Cout_real) else None
    for B in ch.SMALL_B:
        both(run_fwd, f"{name} B={B} forward, route {GENERIC}", fwd, B, geo.Cin, geo.Cout, dt, GENERIC)
        both(run_fwd, f"{name} B={B} mode-1 pack, route {GENERIC}", adj, B, geo.Cin, geo.Cout, dt, GENERIC)
        if two is not None:
            both(run_dgrad, f"{name} B={B} two-tensor, route {GENERIC}", two, B, geo.Cin, geo.Cout, GENERIC, masked=False)
            both(run_dgrad, f"{name} B={B} two-tensor masked, route {GENERIC}", two, B, geo.Cin, geo.Cout, GENERIC, masked=True)


@pytest.mark.parametrize("geo", ch.ODD_TILES, ids=geo_ids(ch.ODD_TILES))
def test_generic_kernel_odd_tile_count_at_wide_slabs(ka_env, geo):
    """(a) bf16, Cout = 80 and 144 (five and nine 16-channel tiles) at B = 256, the batch from which conv_dispatch takes two and
    four tiles per wave for these widths: the last tile is alone in its wave, with no partner for the 16-byte store of a tile
    pair.  Between guard rows first, so that a store past a row's end lands in memory the test owns."""
    select(ka_env, geo.env)
    B, name = ch.B_ODD_TILES, f"conv3x3_kernel {geo.id} B={ch.B_ODD_TILES}"
    fwd, two = ch.fwd_data(B, geo.Cin, geo.Cout), ch.dgrad_data(B, geo.Cin, geo.Cout)
    for guard in (True, False):
        run_fwd(f"{name} forward, route {GENERIC}", fwd, B, geo.Cin, geo.Cout, bf, GENERIC, guard=guard)
        run_dgrad(f"{name} two-tensor, route {GENERIC}", two, B, geo.Cin, geo.Cout, GENERIC, masked=False, guard=guard)
        run_dgrad(f"{name} two-tensor masked, route {GENERIC}", two, B, geo.Cin, geo.Cout, GENERIC, masked=True, guard=guard)


@pytest.mark.parametrize("transform", list(ch.TRANSFORMS))
def test_generic_kernel_transform_combinations(ka_env, transform):
    """(a) Each combination of scale + shift, ReLU and per-board bias the ABI admits, bf16 96 -> 80 and fp32 48 -> 80."""
    select(ka_env, {})
    for dt, Cin in ((bf, 96), (f32, 48)):
        d = ch.fwd_data(ch.B_SMALL, Cin, 80, transform)
        for B in ch.SMALL_B:
            both(run_fwd, f"conv3x3_kernel {Cin}x80 {transform} B={B}, route {GENERIC}", d, B, Cin, 80, dt, GENERIC)


def test_pack_multi_equals_single_packs_on_these_geometries():
    """ka_pack_conv3x3_multi against ka_pack_conv3x3, byte for byte: the forward and the mode-1 pack of two geometries per dtype,
    padded ones included; the single packs are the ones the exact cases above multiply with."""
    for dt in (bf, f32):
        cpk = 32 if dt == bf else 16
        jobs, singles, multis, keep, mx = [], [], [], [], 0
        for geo in (g for g in ch.PACK_MULTI if g.dtype == dt):
            for adjoint in (False, True):
                d = ch.geo_fwd(geo, adjoint=adjoint)
                single = conv_pack(d, dt, geo.Cin, geo.Cout)
                n = 9 * (geo.Cin // cpk) * (geo.Cout // 16) * 64
                multi = torch.full_like(single, 0xA5)
                w = d.w.contiguous().to(DEV)
                jobs.append([w.data_ptr(), multi.data_ptr(), d.w.shape[0], d.w.shape[1], geo.Cout, geo.Cin, int(adjoint), 0])
                singles.append(single); multis.append(multi); keep.append(w)
                mx = max(mx, n)
        table = torch.tensor(jobs, dtype=torch.int64).to(DEV)
        _lib.call("ka_pack_conv3x3_multi", table, len(jobs), mx, _lib.dtype_code(dt), st())
        torch.cuda.synchronize()
        for job, a, b in zip(jobs, singles, multis):
            assert torch.equal(a, b), f"pack {job[2:7]} ({dt}): the multi pack differs from the single pack"


# ------------------------------------------------------------------------------------------------ (b) the training routes
def run_entry(form, entry, B, tag=""):
    C = form.C
    label = f"{form.name} {form.env} C={C} B={B} {entry}{tag}, route {form.routes[entry]}"
    if entry in ("fwd", "fwdt"):
        both(run_fwd, label, ch.train_fwd(C, entry), B, C, C, bf, form.routes[entry])
    elif entry == "keep":
        both(run_fwd, label, ch.train_fwd(C, "fwdt"), B, C, C, bf, form.routes[entry], keep=True)
    else:
        both(run_dgrad, label, ch.train_dgrad(C, entry == "gated"), B, C, C, form.routes[entry], masked=entry != "two")


@pytest.mark.parametrize("form,B", ch.FORM_CASES, ids=[f"{f.name}-B{B}" for f, B in ch.FORM_CASES])
def test_training_routes(ka_env, form, B):
    """(b) bf16, 256 and 128 channels at B = 512 (the dispatch threshold), 513 (the last pair half empty, a corner workgroup with
    one board), 515 (258 pairs on 256 workgroups: two run a second unit) and, on the default route and one producer / consumer
    form, 1027 (every workgroup two units or three, 33 corner workgroups, the last with three boards): every entry the route
    accepts, all boards.  The queries must agree with the table: ka_conv3x3_fwd_keep_supported and
    ka_conv3x3_dgrad_gated_supported say yes exactly where the form lists the entry, and no below 512."""
    select(ka_env, form.env)
    C = form.C
    assert bool(_lib.query("ka_conv3x3_fwd_keep_supported", B, C, C, 1)) == ("keep" in form.routes), f"{form.name}: fwd_keep_supported"
    assert bool(_lib.query("ka_conv3x3_dgrad_gated_supported", B, C, C, 1, 1)) == ("gated" in form.routes), f"{form.name}: gated_supported"
    assert not _lib.query("ka_conv3x3_dgrad_gated_supported", 511, C, C, 1, 1) and not _lib.query("ka_conv3x3_fwd_keep_supported", 511, C, C, 1)
    assert not _lib.query("ka_conv3x3_dgrad_gated_supported", B, C, C, 1, 0), "the gated input comes with the masked epilogue only"
    for entry in form.routes:
        run_entry(form, entry, B)


# ------------------------------------------------------------------------------------------------ (c) rounding
ROUNDING = (
    ("generic", {}, 5, {"fwd": GENERIC, "two": GENERIC, "masked": GENERIC}),
    ("pc2", {}, ch.B_ROUND, {"fwd": ch.IN, "two": ch.IN, "masked": ch.OUT}),
    ("pc2-corner-launch", {"KA_CONV_CORNER_IN": "0"}, ch.B_ROUND, {"fwd": ch.OUT, "two": ch.OUT}),
    ("pc-p3", {"KA_CONV_PC2": "0", "KA_CONV_P": "3"}, ch.B_ROUND, {"fwd": ch.PC, "two": ch.PC, "masked": ch.PC}),
    ("generic-5-tiles", {"KA_CONV_P": "0"}, ch.B_ROUND, {"fwd": ch.GEN, "masked": ch.GEN}),
)


@pytest.mark.parametrize("name,env,B,entries", ROUNDING, ids=[r[0] for r in ROUNDING])
def test_round_to_nearest_even_and_what_the_sums_are_taken_from(ka_env, name, env, B, entries):
    """(c) x (data gradient: in) in -2 .. 2, ternary weights of density 2/3, 256 channels: outputs pass 256, where bf16 holds even
    integers only and every odd one is a tie.  out (and da) must be ref64.to(bfloat16), round-to-nearest-even, bit for bit.

    What the sums are taken from, as the code intends it (conv_epilogue, conv_epilogue_pair, conv_epilogue_masked_pair,
    corner_tile_epilogue and conv3x3_corner_kernel all agree): bsum and sqpart are sums of the fp32 ACCUMULATORS -- of the
    unrounded, and in the masked form unmasked, convolution -- while ep_s1 and ep_s2 are sums of the masked value AS STORED,
    d = float(bf16(acc)) where the mask is set: sum d and sum d (y - mean) invstd.  conv_helpers.dgrad_data builds its
    references that way, and every route is held to it: the generic kernel, the two-board kernel with the corner inside and
    behind it, the producer / consumer kernel, and conv3x3_kernel<.., 5> with the corner launch."""
    select(ka_env, env)
    fwd, dg = ch.round_fwd(), ch.round_dgrad()
    ties = ((fwd.out[:B].abs() > 256) & (fwd.out[:B] % 2 == 1)).sum(), ((dg.dh[:B].abs() > 256) & (dg.dh[:B] % 2 == 1)).sum()
    assert int(ties[0]) > 0 or B < 512
    assert int(ties[1]) > 0 or B < 512
    # rounded and unrounded sums must really differ on these data, or the case decides nothing
    if B >= 512:
        assert not torch.equal(fwd.out[:B].to(bf).double().sum(1), fwd.bsum[:B].double())
        assert not torch.equal(dg.da[:B].double().sum(1), (dg.dh[:B].double() * (dg.da[:B] != 0)).sum(1))
    for entry, expected in entries.items():
        label = f"rounding {name} {env} B={B} {entry}, route {expected}"
        if entry == "fwd":
            both(run_fwd, label, fwd, B, 256, 256, bf, expected)
        else:
            both(run_dgrad, label, dg, B, 256, 256, expected, masked=entry == "masked")


# ------------------------------------------------------------------------------------------------ (d) Gaussian data
SEQ_FACTOR = 4      # the project's margin (tests/test_hip_wgrad_exact.py): a matrix pipe that truncates where the CPU rounds x a twofold spread between orders
GAUSSIAN = (("generic-bf16-B37", bf, 37, {}, GENERIC, GENERIC), ("pc2-bf16-B515", bf, 515, {}, ch.IN, ch.IN),
            ("generic-f32-B5", f32, 5, {}, GENERIC, None))


@pytest.mark.parametrize("name,dt,B,env,fwd_routes,two_routes", GAUSSIAN, ids=[g[0] for g in GAUSSIAN])
def test_accumulation_error_on_gaussian_data(ka_env, name, dt, B, env, fwd_routes, two_routes):
    """(d) bf16-rounded N(0, 1) activations and N(0, 1) / (3 sqrt C) weights, 256 channels (fp32 gets the same values): the
    forward and the plain two-tensor data gradient (fp32, which has no two-tensor entry: the mode-1 pack through ka_conv3x3_fwd),
    every element of every board:
        bf16:  |got - ref64| <= 2^-8 |ref64| + SEQ_FACTOR x e_seq        (half a bf16 ulp, then the accumulation)
        fp32:  |got - ref64| <= SEQ_FACTOR x e_seq
    e_seq = the largest error, over the first 16 boards, of a float32 CPU accumulation of the same products one at a time, tap
    by tap and channel by channel.  dy_out of the two-tensor form must be the bf16 of the exact a k0 + in2 k2 to the bit
    (conv_helpers.gaussian_case says why that is well defined).

    Measured on an MI355X (e_seq is 1.0e-6 .. 1.3e-6 max|ref| in every case).  fp32: max err / e_seq.  bf16: the raw error is the
    output rounding (about 2500 e_seq), so the figure is the largest part of an element's error beyond 2^-8 |ref64|, in e_seq:
      generic route, bf16, B = 37:          forward 0.06, data gradient 0.05
      default route (pc2), bf16, B = 515:   forward 0.11, data gradient 0.10
      generic route, fp32, B = 5:           forward 1.13, data gradient 1.00"""
    select(ka_env, env)
    C = 256
    x, in2, w, k, dy = ch.gaussian_case(B, C, 3)
    code, rows = _lib.dtype_code(dt), _lib.query("ka_conv3x3_sqpart_rows", B)
    cases = [("forward", x, False, ch.conv64(x, w, False))]
    cases.append(("data gradient", dy, True, ch.conv64(dy, w, True)))
    for what, h, adjoint, ref in cases:
        e_seq, scale = ch.seq_f32_error(h, w, adjoint, ref), ch.amax(ref)
        wp = pack(w, dt, int(adjoint), C, C)
        out = torch.full((B, 81, C), float("nan"), dtype=dt, device=DEV)
        bsum = torch.full((B, C), float("nan"), device=DEV)
        if adjoint and dt == bf:
            dyo = torch.full((B, 81, C), float("nan"), dtype=bf, device=DEV)
            counted(name, two_routes, "ka_conv3x3_dgrad_fused", x.to(DEV, bf), in2.to(DEV, bf), k.to(DEV), dyo, wp, out, bsum, None, None, None,
                    None, None, None, None, B, C, C, 1, st())
            require_equal(f"{name}: dy_out", dyo, dy.to(DEV, bf), B)
        else:
            sq = torch.full((rows, C), float("nan"), device=DEV)
            counted(name, fwd_routes, "ka_conv3x3_fwd", h.to(DEV, dt), wp, out, None, None, None, 0, bsum, sq, B, C, C, code, st())
        refd = ref.to(DEV)
        err = (out.double() - refd).abs()
        assert bool(torch.isfinite(err).all()), f"{name} {what}: an element was not written"
        half_ulp = 2.0 ** -8 * refd.abs() if dt == bf else torch.zeros_like(refd)
        excess = float((err - half_ulp).max())
        print(f"\n{name} {what}: e_seq = {e_seq:.3e} = {e_seq / scale:.3e} max|ref|; max err {float(err.max()):.3e} = "
              f"{float(err.max()) / e_seq:.2f} e_seq; beyond half a bf16 ulp of the reference: {max(excess, 0.0) / e_seq:.2f} e_seq")
        over = err > half_ulp + SEQ_FACTOR * e_seq
        if bool(over.any()):
            b, p, c = (int(v) for v in torch.unravel_index((err - half_ulp).argmax(), err.shape))
            pytest.fail(f"{name} {what}: {int(over.sum())} elements beyond the bound, worst (board, square, channel) = ({b}, {p}, {c}): "
                        f"got {float(out[b, p, c])}, reference {float(refd[b, p, c])}, e_seq {e_seq:.3e}")
        # the per-board sums are taken from the accumulators: 81 of them, each within the accumulation bound
        berr = float((bsum.double() - refd.sum(1)).abs().max())
        assert berr <= 81 * SEQ_FACTOR * e_seq, f"{name} {what}: bsum error {berr:.3e}"
