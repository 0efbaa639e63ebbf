"""CPU proofs for tests/conv_helpers.py, the oracle of tests/test_hip_conv_exact.py: the fp64 reference equals a second,
independent formulation (nine shifted matmuls, the adjoint as the flipped and transposed kernel -- the pack's mode-1 convention);
every case of every list meets the two exactness conditions; one changed product changes the reference; and a float32
convolution of the same integers equals the fp64 one bit for bit, which is the order-independence the GPU test relies on."""
import pytest
import torch
import torch.nn.functional as F

import conv_helpers as ch


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("Cin,Cout", [(32, 48), (50, 16), (96, 80)])
def test_oracle_equals_nine_shifted_matmuls(Cin, Cout, adjoint):
    g = ch.gen(9, Cin, Cout, adjoint)
    h = ch.ints(g, 3, 3, ch.BOARD, Cin)
    w = ch.ints(g, 2, *((Cin, Cout, 3, 3) if adjoint else (Cout, Cin, 3, 3)))
    assert torch.equal(ch.conv64(h, w, adjoint), ch.conv_taps64(h, w, adjoint))


def test_adjoint_is_the_transpose_of_the_forward():
    """<conv(x, w), dy> == <x, adjoint(dy, w)> exactly on integers: conv64's adjoint is the data gradient of its forward."""
    g = ch.gen(10)
    x, dy, w = ch.ints(g, 2, 2, ch.BOARD, 32), ch.ints(g, 2, 2, ch.BOARD, 48), ch.ints(g, 1, 48, 32, 3, 3)
    assert float((ch.conv64(x, w, False) * dy.double()).sum()) == float((x.double() * ch.conv64(dy, w, True)).sum())


def test_pack_mode_one_convention():
    """One weight entry w[c, n, ky, kx] of the forward layer: the adjoint's output at square p, channel n takes dy at square
    p + tap with tap = 8 - (3 ky + kx), i.e. the pack's `8 - tap`."""
    w = torch.zeros(16, 16, 3, 3)
    w[5, 7, 0, 2] = 1.0                                        # forward tap 2 = (dy -1, dx +1)
    dy = torch.zeros(1, ch.BOARD, 16)
    dy[0, 4 * 9 + 4, 5] = 1.0
    out = ch.conv64(dy, w, True)
    hit = torch.nonzero(out)
    # flipped tap 6 = (+1, -1): the output square whose (+1, -1) neighbour is (4, 4) is (3, 5)
    assert hit.tolist() == [[0, 3 * 9 + 5, 7]] and float(out[0, 3 * 9 + 5, 7]) == 1.0


CASES = ch.all_case_builders()


@pytest.mark.parametrize("label,build", CASES, ids=[c[0].replace(" ", "-") for c in CASES])
def test_every_case_meets_the_exactness_conditions(label, build):
    """Building a case asserts both conditions (conv_helpers.check_exact): every fp32 partial sum below 2^24, every bf16-stored
    value an integer of at most 256 (the rounding cases: allowed past 256, sums bounded by their real size)."""
    d = build()
    out = d.out if isinstance(d, ch.Fwd) else d.dh
    assert ch.amax(out) > 0
    if label.startswith("round"):
        assert ch.amax(out) > ch.BF16_INT, "the rounding case must pass 256"
        odd = (out.abs() > ch.BF16_INT) & (out % 2 == 1)
        print(f"{label}: max |ref| {ch.amax(out)}, {int(odd.sum())} ties")
        assert int(odd.sum()) >= 10, "the rounding case needs ties"             # (forward: 19, at 4.6 sigma; the data gradient: many)
    else:
        assert ch.amax(out) <= ch.BF16_INT


def test_training_magnitudes_as_measured():
    """max |ref| at the largest batch stays where the densities were chosen to put it."""
    for C in (256, 128):
        for entry in ("fwd", "fwdt"):
            print(C, entry, ch.amax(ch.train_fwd(C, entry).out))
        for gated in (False, True):
            d = ch.train_dgrad(C, gated)
            print(C, "gated" if gated else "two", ch.amax(d.dh), ch.amax(d.dy))
            assert ch.amax(d.dy) == (5 if gated else 3)


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
def test_one_changed_product_changes_the_reference(adjoint):
    """A single weight entry, a single input square: at the corner square 80 and at an interior square, the reference moves in
    exactly the outputs that product feeds."""
    d = ch.fwd_data(2, 32, 48, "plain", adjoint=adjoint)
    base = ch.conv64(d.h, d.w, adjoint)
    # one weight entry +1: every output of that output channel that has the tap on the board moves by h
    w2 = d.w.clone()
    w2[3, 5, 1, 1] += 1.0                                      # the centre tap: all 81 squares
    delta = ch.conv64(d.h, w2, adjoint) - base
    cin, cout = (3, 5) if adjoint else (5, 3)
    assert torch.equal(delta[:, :, cout], d.h.double()[:, :, cin])
    assert ch.amax(delta[:, :, :cout]) == 0 and ch.amax(delta[:, :, cout + 1:]) == 0
    for square in (80, 40):
        h2 = d.h.clone()
        h2[1, square, 7] += 1.0
        delta = ch.conv64(h2, d.w, adjoint) - base
        touched = torch.nonzero(delta.abs().sum(2))
        assert set(touched[:, 0].tolist()) == {1}
        rows, cols = square // 9, square % 9
        neighbours = {9 * r + c for r in range(rows - 1, rows + 2) for c in range(cols - 1, cols + 2) if 0 <= r < 9 and 0 <= c < 9}
        assert set(touched[:, 1].tolist()) <= neighbours and square in set(touched[:, 1].tolist())
        assert ch.amax(delta) == 1.0 and len(neighbours) == (4 if square == 80 else 9)


@pytest.mark.parametrize("kind", ["fwd", "fwdt", "two", "gated", "round"])
def test_float32_convolution_of_the_integers_is_exact(kind):
    """The order-independence claim: PyTorch's float32 convolution (another summation order again) gives the fp64 result bit
    for bit on the operands of the training cases (a 64-board slice)."""
    B = 64
    if kind in ("fwd", "fwdt"):
        d = ch.train_fwd(256, kind, B)
        got = ch.nhwc(F.conv2d(ch.nchw(d.h), d.w, padding=1))
        ref = d.out
    elif kind == "round":
        d = ch.round_fwd(B)
        got = ch.nhwc(F.conv2d(ch.nchw(d.h), d.w, padding=1))
        ref = d.out
    else:
        d = ch.train_dgrad(256, kind == "gated", B)
        got = ch.nhwc(torch.nn.grad.conv2d_input((B, 256, 9, 9), d.w, ch.nchw(d.dy), padding=1))
        ref = d.dh
    assert got.dtype == torch.float32 and torch.equal(got, ref)


def test_masked_reference_is_decided_exactly():
    """ep_scale * y + ep_shift is never within 0.5 of zero, da is dh where it is positive and zero elsewhere, and the sums are
    the sums of da over the squares."""
    d = ch.train_dgrad(128, False, 8)
    pre = d.y.double() * d.ep[0].double() + d.ep[1].double()
    assert float(pre.abs().min()) >= 0.5
    assert torch.equal(d.da.double(), torch.where(pre > 0, d.dh.double(), torch.zeros(()).double()))
    assert torch.equal(d.s1, d.da.double().sum(1)) and torch.equal(d.bsum.double(), d.dh.double().sum(1))
    frac = float((pre > 0).double().mean())
    assert 0.3 < frac < 0.7


def test_explain_names_the_place():
    exp = torch.zeros(515, ch.BOARD, 32)
    got = exp.clone()
    got[514, 80, 17] = 3.0
    msg = ch.explain("x", got, exp, 515)
    for part in ("1 of", "(514, 80, 17)", "square 80", "last board", "16-channel tile 1", "past the first 512"):
        assert part in msg, (part, msg)
    got[3, 5, 0] = float("nan")
    assert "not confined" in ch.explain("x", got, exp, 515) or "2 of" in ch.explain("x", got, exp, 515)


def test_take_slices_boards_only():
    d = ch.train_dgrad(128, True, 513)
    assert d.a.shape[0] == 513 and d.ga.shape == (2, 513, 128) and d.k.shape == (384,) and d.w.shape == (128, 128, 3, 3)
    assert d.s1.shape == (513, 128) and d.a.is_contiguous()
