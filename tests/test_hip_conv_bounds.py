"""Guard-band tests of the tower convolutions at odd batch sizes: every tensor with a per-board leading dimension is handed to
the library as the middle of a larger allocation, with guard rows before and after it.  Output guards hold a bit pattern that
must survive the call bit for bit; input guards are zero in one run and NaN in another, and the outputs of the two runs must
be bit-identical and finite.  The guard rows are larger than any overrun a kernel can make (one board), so every access stays
inside memory the test owns, and no test depends on a fault.  The ragged edge -- boards 0, 1, B-2 and B-1, the last pair half
empty at odd B -- is held to an fp64 CPU reference computed from the bf16-rounded operands."""
import functools

import pytest
import torch

from keisei_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 4                                                        # guard rows (boards) before and after every guarded tensor
PATTERN = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FC0A5A5)}


def st():
    return _lib.stream_ptr()


def guarded(shape, dtype, fill, g=G, off=0, device=DEV):
    """(full, mid): full has g extra rows of the leading dimension before and after; mid = full[g:-g] is contiguous.
    fill: a float, or "pattern" for the output guard bit pattern.  off (one-dimensional tensors only): mid starts `off`
    elements later, full is 8 elements longer, and the elements on both sides of mid are guards all the same."""
    assert off == 0 or (len(shape) == 1 and 0 < off < 8)
    full_shape = (shape[0] + 2 * g + (8 if off else 0), *shape[1:])
    if fill == "pattern":
        it, v = PATTERN[dtype]
        full = torch.full(full_shape, v, dtype=it, device=device).view(dtype)
    else:
        full = torch.full(full_shape, fill, dtype=dtype, device=device)
    return full, full[g + off:g + off + shape[0]]


def bits(t):
    return t.view(PATTERN[t.dtype][0])


def middle(full, g=G, off=0):
    return full[g + off:full.shape[0] - g - (8 - off if off else 0)]


def guards_intact(full, g=G, off=0):
    it, v = PATTERN[full.dtype]
    b = full.view(it)
    end = full.shape[0] - g - (8 - off if off else 0)
    return bool((b[:g + off] == v).all()) and bool((b[end:] == v).all())


def _spec(entry, first):
    """(what, guard rows, off) of an entry of run_guarded; first = 1: a tensor or (tensor[, g[, off]]), first = 2: (shape, dtype[,
    g[, off]]), what = (shape, dtype).  The default is G rows and no offset."""
    if first == 2:
        return (entry[0], entry[1]), (entry[2] if len(entry) > 2 else G), (entry[3] if len(entry) > 3 else 0)
    if isinstance(entry, tuple):
        return entry[0], entry[1], (entry[2] if len(entry) > 2 else 0)
    return entry, G, 0


def run_guarded(call, inputs, outputs, in_fill, inout=None, device=DEV):
    """inputs: name -> tensor (leading dimension guarded) or (tensor, guard rows[, off]); outputs: name -> (shape, dtype[, guard
    rows[, off]]); inout: like inputs, for tensors the call updates in place (pattern guards).  Returns name -> full tensor."""
    bufs, fulls = {}, {}
    for n, e in inputs.items():
        t, g, off = _spec(e, 1)
        full, mid = guarded(tuple(t.shape), t.dtype, in_fill, g, off, device)
        mid.copy_(t)
        bufs[n] = mid
    for n, e in (inout or {}).items():
        t, g, off = _spec(e, 1)
        fulls[n], bufs[n] = guarded(tuple(t.shape), t.dtype, "pattern", g, off, device)
        bufs[n].copy_(t)
    for n, e in outputs.items():
        (shape, dt), g, off = _spec(e, 2)
        fulls[n], bufs[n] = guarded(shape, dt, "pattern", g, off, device)
    sync = torch.device(device).type == "cuda"
    if sync:
        torch.cuda.synchronize()
    call(bufs)
    if sync:
        torch.cuda.synchronize()
    return fulls


def check_guarded(call, inputs, outputs, finite=None, inout=None, valid=None, device=DEV):
    """Both runs: output guards intact; every output's middle finite (the names in `finite`, default all; valid: name -> a
    function that cuts the region that must be finite out of the middle, for outputs with pad columns) and bit-identical
    between zero and NaN input guards.  Returns the middles of the NaN-guard run."""
    runs = [run_guarded(call, inputs, outputs, f, inout, device) for f in (0.0, float("nan"))]
    where = {n: _spec(e, 2)[1:] for n, e in outputs.items()}
    where.update({n: _spec(e, 1)[1:] for n, e in (inout or {}).items()})
    for fill, res in zip(("zero", "NaN"), runs):
        for n, full in res.items():
            assert guards_intact(full, *where[n]), f"{n}: guard rows overwritten ({fill} input guards)"
    mids = [{n: middle(full, *where[n]) for n, full in res.items()} for res in runs]
    for n in where:
        if finite is None or n in finite:
            region = (valid or {}).get(n, lambda t: t)
            assert bool(torch.isfinite(region(mids[1][n]).float()).all()), f"{n}: non-finite (or unwritten) element in the valid region"
            assert torch.equal(bits(mids[0][n]), bits(mids[1][n])), f"{n}: depends on memory past the tensors"
    return mids[1]


# ------------------------------------------------------------------------------------------------ fp64 references
@functools.lru_cache(maxsize=None)
def weights(C):
    """(w fp32 cpu, forward pack, data-gradient pack): shared by every case of a channel count."""
    g = torch.Generator().manual_seed(C)
    w = torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)
    packs = []
    for mode in (0, 1):
        wp = torch.empty(9 * (C // 32) * (C // 16) * 1024, dtype=torch.uint8, device=DEV)
        _lib.call("ka_pack_conv3x3", w.to(DEV), wp, C, C, C, C, mode, 1, st())
        packs.append(wp)
    torch.cuda.synchronize()
    return w, packs[0], packs[1]


def conv_ref(xp, w, adjoint):
    """xp: (n, 81, C) fp64 -> (n, 81, C) fp64: the convolution (or, adjoint, the data gradient) with the bf16-rounded weights."""
    n, _, C = xp.shape
    x = xp.reshape(n, 9, 9, C).permute(0, 3, 1, 2)
    wd = w.to(torch.bfloat16).double()
    y = torch.nn.grad.conv2d_input(x.shape, wd, x, padding=1) if adjoint else torch.nn.functional.conv2d(x, wd, padding=1)
    return y.permute(0, 2, 3, 1).reshape(n, 81, C)


def ragged(B):
    return sorted({0, 1, B - 2, B - 1} & set(range(B)))


def cpu64(t, idx):
    return t[idx].double().cpu()


def assert_rel(got, ref, tol, what):
    """per board: max |got - ref| <= tol * max |ref| of that board"""
    for i in range(ref.shape[0]):
        scale = float(ref[i].abs().max())
        err = float((got[i].double() - ref[i]).abs().max())
        assert err <= tol * scale + 1e-30, f"{what}, board row {i}: max err {err:.3e} > {tol:.1e} x {scale:.3e}"


def assert_sums(got, ref, what):
    """per-board sums: the class of the existing tests' close(..., float32, k=200), scaled by the boards' max |ref|"""
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got.double() - ref).abs().max())
    assert err <= 2e-5 * 200 * scale, f"{what}: max err {err:.3e} > {4e-3 * scale:.3e}"


# ------------------------------------------------------------------------------------------------ the cases
ROUTES = {
    "default": {},
    "corner_launch": {"KA_CONV_CORNER_IN": "0"},
    "stag": {"KA_CONV_PC2_STAG": "1"},
    "skip": {"KA_CONV_PC2_SKIP": "1"},
    "no_pc2": {"KA_CONV_PC2": "0"},
    "no_pc": {"KA_CONV_P": "0"},
}
ODD, EVEN, SMALL = (513, 515, 4097), (512, 514), (3, 37, 129)
CASES = ([(256, r, B) for r in ROUTES for B in ODD + EVEN] + [(128, r, B) for r in ("default", "no_pc2") for B in ODD + EVEN]
         + [(256, "default", B) for B in SMALL] + [(128, "default", B) for B in SMALL])


def operands(B, C):
    g = torch.Generator(device=DEV).manual_seed(1000 * C + B)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    pos = lambda *s: torch.rand(*s, device=DEV, generator=g) + 0.5
    return dict(
        x=rnd(B, 81, C).to(torch.bfloat16), x2=rnd(B, 81, C).to(torch.bfloat16), y=rnd(B, 81, C).to(torch.bfloat16),
        gb=0.1 * rnd(B, C), ga=torch.cat([pos(1, B, C), 0.1 * rnd(1, B, C)]),
        sc=pos(C), sh=0.1 * rnd(C), k=torch.cat([pos(C), 0.1 * rnd(C), 0.2 * rnd(C)]), mu=0.1 * rnd(C), istd=pos(C))


@pytest.mark.parametrize("C,route,B", CASES, ids=[f"C{c}-{r}-B{b}" for c, r, b in CASES])
def test_tower_conv_stays_inside_its_tensors(ka_env, C, route, B):
    """ka_conv3x3_fwd (plain; scale / shift / per-board bias / ReLU), ka_conv3x3_fwd_keep, ka_conv3x3_dgrad_fused (plain and masked
    epilogue) and ka_conv3x3_dgrad_fused_gated on guarded tensors, each route of conv_dispatch, odd and even batches: nothing
    written or read outside the tensors, and the ragged edge equal to the fp64 reference."""
    for name, value in ROUTES[route].items():
        ka_env.set(name, value)
    w, wp, wpd = weights(C)
    o = operands(B, C)
    a, sc, sh, k, mu, istd = o["x"], o["sc"], o["sh"], o["k"], o["mu"], o["istd"]
    act, vec, rows = (B, 81, C), (B, C), _lib.query("ka_conv3x3_sqpart_rows", B)
    bf, f32 = torch.bfloat16, torch.float32
    R = ragged(B)
    x64 = cpu64(a, R)

    # ---- forward, plain
    m = check_guarded(lambda t: _lib.call("ka_conv3x3_fwd", t["x"], wp, t["out"], None, None, None, 0, t["bsum"], t["sq"], B, C, C, 1, st()),
                      {"x": a}, {"out": (act, bf), "bsum": (vec, f32), "sq": ((rows, C), f32)})
    ref = conv_ref(x64, w, False)
    assert_rel(cpu64(m["out"], R), ref, 6e-3, "fwd out")
    assert_sums(cpu64(m["bsum"], R), ref.sum(1), "fwd bsum")
    assert_sums(cpu64(m["sq"], R), (ref ** 2).sum(1), "fwd sqpart")

    # ---- forward with scale / shift / per-board bias / ReLU; with x' kept where the two-board kernel takes it
    keep = bool(_lib.query("ka_conv3x3_fwd_keep_supported", B, C, C, 1))
    outs = {"out": (act, bf), "bsum": (vec, f32), "sq": ((rows, C), f32)}
    if keep:
        outs["xk"] = (act, bf)
        call = lambda t: _lib.call("ka_conv3x3_fwd_keep", t["x"], wp, t["out"], sc, sh, t["gb"], 1, t["bsum"], t["sq"], t["xk"], B, C, C, 1, st())
    else:
        call = lambda t: _lib.call("ka_conv3x3_fwd", t["x"], wp, t["out"], sc, sh, t["gb"], 1, t["bsum"], t["sq"], B, C, C, 1, st())
    m = check_guarded(call, {"x": a, "gb": o["gb"]}, outs)
    xp = (torch.relu(x64 * sc.double().cpu() + sh.double().cpu()) + cpu64(o["gb"], R)[:, None, :]).to(bf).double()
    ref = conv_ref(xp, w, False)
    assert_rel(cpu64(m["out"], R), ref, 6e-3, "fwd (transform) out")
    assert_sums(cpu64(m["bsum"], R), ref.sum(1), "fwd (transform) bsum")
    assert_sums(cpu64(m["sq"], R), (ref ** 2).sum(1), "fwd (transform) sqpart")
    if keep:
        assert_rel(cpu64(m["xk"], R), xp, 2.0 ** -7, "fwd_keep x_out")

    # ---- data gradient: dy = in*k0 + k1 + in2*k2 written back, out = the adjoint convolution of dy [masked]
    k64 = k.double().cpu()
    dy_ref = (x64 * k64[:C] + k64[C:2 * C] + cpu64(o["x2"], R) * k64[2 * C:]).to(bf).double()
    dh_ref = conv_ref(dy_ref, w, True)
    m = check_guarded(lambda t: _lib.call("ka_conv3x3_dgrad_fused", t["x"], t["x2"], k, t["dy"], wpd, t["out"], t["bsum"], None, None, None,
                                          None, None, None, None, B, C, C, 1, st()),
                      {"x": a, "x2": o["x2"]}, {"out": (act, bf), "dy": (act, bf), "bsum": (vec, f32)})
    assert_rel(cpu64(m["dy"], R), dy_ref, 2.0 ** -7, "dgrad dy_out")
    assert_rel(cpu64(m["out"], R), dh_ref, 6e-3, "dgrad out")
    assert_sums(cpu64(m["bsum"], R), dh_ref.sum(1), "dgrad bsum")

    def masked_ref(dh, y):
        pre = y * sc.double().cpu() + sh.double().cpu()
        da = dh * (pre > 0)
        s1 = da.sum(1)
        s2 = (da * (y - mu.double().cpu()) * istd.double().cpu()).sum(1)
        return da, s1, s2, pre.abs() > 1e-4                  # (elements whose mask the fp32 kernel might decide the other way: not compared)

    def check_masked(m, dy_ref, what):
        dh = conv_ref(dy_ref, w, True)
        da, s1, s2, sure = masked_ref(dh, cpu64(o["y"], R))
        assert_rel(cpu64(m["dy"], R), dy_ref, 2.0 ** -7, what + " dy_out")
        assert_rel(cpu64(m["out"], R) * sure, da * sure, 6e-3, what + " da")
        assert_sums(cpu64(m["bsum"], R), dh.sum(1), what + " bsum")
        assert_sums(cpu64(m["e1"], R), s1, what + " ep_s1")
        assert_sums(cpu64(m["e2"], R), s2, what + " ep_s2")

    ep_outs = {"out": (act, bf), "dy": (act, bf), "bsum": (vec, f32), "e1": ((rows, C), f32), "e2": ((rows, C), f32)}
    m = check_guarded(lambda t: _lib.call("ka_conv3x3_dgrad_fused", t["x"], t["x2"], k, t["dy"], wpd, t["out"], t["bsum"], t["y"], sc, sh,
                                          mu, istd, t["e1"], t["e2"], B, C, C, 1, st()),
                      {"x": a, "x2": o["x2"], "y": o["y"]}, ep_outs)
    check_masked(m, dy_ref, "dgrad masked")

    # ---- gated data gradient: dz = du*gate + add (never rounded), dy = dz*k0 + k1 + in2*k2
    if _lib.query("ka_conv3x3_dgrad_gated_supported", B, C, C, 1, 1):
        m = check_guarded(lambda t: _lib.call("ka_conv3x3_dgrad_fused_gated", t["x"], t["ga"], t["x2"], k, t["dy"], wpd, t["out"], t["bsum"],
                                              t["y"], sc, sh, mu, istd, t["e1"], t["e2"], B, C, C, 1, st()),
                          {"x": a, "ga": o["ga"].reshape(2 * B, C), "x2": o["x2"], "y": o["y"]}, ep_outs)
        ga = o["ga"].double().cpu()[:, R]
        dz = x64 * ga[0][:, None, :] + ga[1][:, None, :]
        check_masked(m, (dz * k64[:C] + k64[C:2 * C] + cpu64(o["x2"], R) * k64[2 * C:]).to(bf).double(), "gated")
    else:
        assert route in ("no_pc2", "no_pc") or B < 512, "the gated form should be taken here"


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
@pytest.mark.parametrize("B", [515, 4097])
def test_weight_gradient_at_odd_batch_stays_inside_its_tensors(B, dtn):
    """ka_conv3x3_wgrad on dy / x of odd B (bf16: the lean kernel; fp32), guarded dy, x, dw and slab: guards intact, dw the
    same with zero and NaN input guards, and equal to dy^T im2col(x) in fp64."""
    C = 256
    dt = torch.bfloat16 if dtn == "bf16" else torch.float32
    g = torch.Generator(device=DEV).manual_seed(B + 5)
    x = torch.randn(B, 81, C, device=DEV, generator=g).to(dt)
    dy = (torch.randn(B, 81, C, device=DEV, generator=g) / 9).to(dt)
    ns = _lib.query("ka_wgrad_splits", B, C, C, 0)
    m = check_guarded(lambda t: _lib.call("ka_conv3x3_wgrad", t["dy"], t["x"], None, None, None, 0, t["slab"], t["dw"], B, C, C, C, 0, 0,
                                          _lib.dtype_code(dt), st()),
                      {"dy": dy, "x": x}, {"dw": ((C, C, 3, 3), torch.float32), "slab": ((ns * 9 * C, C), torch.float32)}, finite={"dw"})
    cols = torch.nn.functional.unfold(x.double().reshape(B, 9, 9, C).permute(0, 3, 1, 2), 3, padding=1)     # (B, C*9, 81)
    ref = (dy.double().reshape(B * 81, C).t() @ cols.transpose(1, 2).reshape(B * 81, C * 9)).reshape(C, C, 3, 3).cpu()
    del cols
    err, scale = float((m["dw"].double().cpu() - ref).abs().max()), float(ref.abs().max())
    assert err <= (2e-3 if dt == torch.bfloat16 else 3e-5) * scale, (err, scale)


def test_forward_conv_past_two_gigabytes():
    """ka_conv3x3_fwd on the default 256-channel route (conv3x3_pc2_kernel with the in-kernel corner) at B = 51783: the input and
    output tensors are 2^31 + 61 KB each.  The staging waves address a pair through a descriptor based at its first board, the
    epilogues through 64-bit board products: boards on both sides of the 2^31-byte mark and the last (half-empty) pair equal to
    the fp64 reference, every per-board sum written."""
    B, C = 51783, 256
    w, wp, _ = weights(C)
    assert B * 81 * C * 2 > 2 ** 31 and B % 2 == 1
    g = torch.Generator(device=DEV).manual_seed(B)
    x = torch.empty(B, 81, C, dtype=torch.bfloat16, device=DEV)
    for i in range(0, B, 8192):                              # (fp32 noise a slice at a time: no 4 GB temporary)
        n = min(8192, B - i)
        x[i:i + n] = torch.randn(n, 81, C, device=DEV, generator=g).to(torch.bfloat16)
    fo, out = guarded((B, 81, C), torch.bfloat16, "pattern")
    fb, bsum = guarded((B, C), torch.float32, "pattern")
    _lib.call("ka_conv3x3_fwd", x, wp, out, None, None, None, 0, bsum, None, B, C, C, 1, st())
    torch.cuda.synchronize()
    assert guards_intact(fo) and guards_intact(fb)
    assert bool(torch.isfinite(bsum).all())
    board = 81 * C * 2
    R = [0, 2 ** 31 // board - 1, 2 ** 31 // board, 2 ** 31 // board + 1, B - 1]       # 51780 / 51781 straddles byte 2^31 / 51782
    ref = conv_ref(cpu64(x, R), w, False)
    assert_rel(cpu64(out, R), ref, 6e-3, "fwd out past 2 GB")
    assert_sums(cpu64(bsum, R), ref.sum(1), "fwd bsum past 2 GB")
    del x, fo, out


def test_eval_per_layer_path_keeps_boards_independent_at_odd_batch(monkeypatch):
    """bf16 eval forward of a 3 x 256 model on the per-layer path (KA_TOWER=0: every tower conv on conv3x3_pc2_kernel at these
    batch sizes): board 515 of 516 all zeros or all NaN leaves rows 0..514 bit-identical and finite; the first 515 boards alone
    (odd: the last pair half empty) give the same rows bit for bit."""
    from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
    from oracle import keisei_oracle as orc

    monkeypatch.setenv("KA_TOWER", "0")
    monkeypatch.setenv("KA_EVAL_GRAPH", "0")
    shape = orc.NetShape(3, 256)
    m = SEResNetModel(SEResNetParams(**shape.__dict__))
    m.load_state_dict(orc.init_like_state_dict(shape), strict=True)
    m.to(DEV)
    m.configure_amp(True, torch.bfloat16, "cuda")
    m.eval()
    obs = torch.randn(516, 50, 9, 9, generator=torch.Generator().manual_seed(516)).to(DEV)

    def run(o):
        with torch.no_grad():
            r = m(o)
        torch.cuda.synchronize()
        return [t.float()[:515].clone() for t in (r.policy_logits, r.value_logits, r.score_lead)]

    runs = []
    for fill in (0.0, float("nan")):
        o = obs.clone()
        o[515] = fill
        runs.append(run(o))
    runs.append(run(obs[:515].contiguous()))
    for name, a, b, c in zip(("policy", "value", "score"), *runs):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and bool(torch.isfinite(c).all()), name
        assert torch.equal(a, b), f"{name}: a board's output depends on another board"
        assert torch.equal(a, c), f"{name}: 515 boards differ from the first 515 of 516"
