"""The eval tower, the grouped stem and the grouped heads (csrc/tower.hip) against the oracles of tests/tower_helpers.py, called
through the C ABI with pointer tables the test builds itself, so that G, R, P, V, S and cin are free of any model class.

Tier 1: integer operands, the kernel must equal the float64 reference to the bit (x_out, the max quarter of pool_out, zeros in
the last quarter).  Tier 2: real operands, one bf16 rounding between the float64 value and x_out, held to the project's bound
(board_helpers.bound_of: MARGIN x e32 + 2**-8 |ref| for a bf16 output, MARGIN x e32 for an fp32 one); pool_out is held to the
statistics of the kernel's own x_out.  Every output buffer is handed over full of NaN.

Which case runs which path of tower.hip:
  global chain, first phase    G = 8 (one row per wave, rows 1..7 of a wave's eight clamped to G - 1 and their stores guarded),
                               G = 24 (clamp + guard inside the first trip), G = 72 / 200 (a second / fourth trip of jb += 64,
                               the rotation (8 b) % G wrapping inside a trip), G = 256 (kHid full): test_exact_tower[conv-*],
                               test_global_chain_tier2[*]; B = 5 gives rot1 = 0, 8, 16, 24, 32 and rot2 = 0 .. 64
  global chain, second phase   n = G / 2 = 4 (one f32x4 per half row) .. 128; tid < 2C at C = 128: the same cases
  SE hidden                    R = 1, 3 (clamped rows), 16, 36 (second trip of jb += 32), 64 (kSeHid full): test_exact_tower[se-*],
                               test_se_chain_tier2[*]
  SE output                    R % 4 != 0 (R = 1, 3: the scalar loop) and R % 4 == 0 (16, 36, 64: f32x4): the same cases
  conv1 / conv2                C = 256 (all eight waves, two 128-channel chunks) and C = 128 (waves 4..7 skip the MFMA loop):
                               test_exact_tower[conv-*]; nblocks = 3 hands the recomputed max to the next block's chain
  ka_tower_eval                the K = 1 cases at C = 256 run through both entry points
  pool_stats                   constant planes (std exactly 0), an all-zero plane, the maximum on square 80 alone:
                               test_se_chain_tier2, test_global_chain_tier2 (every plane constant), test_stem_affine_tier2
  stem                         cin = 1, 46 (the VecEnv default), 50, 127, 128 (no zero padding), obs allocated with exactly cin
                               planes and a NaN guard band behind it: test_stem_exact, test_stem_affine_tier2
  heads                        P = 1, 7, 32; (V, S) = (1, 1), (3, 65), (200, 130), (512, 512): test_heads
  unseated boards              model_of = -1 and = K: test_unseated_boards_*, test_heads (boards 1 and 4)

Measured on an MI355X: 96 test cases, the whole file 2.6 s wall, no test above 0.3 s.  Tier 1 is equal to the bit in every
case.  Worst error / bound of tier 2 per kernel (measured values, not targets; the bound is the imported one):
  tower global chain   0.9925  (gp-C256-G256-R16)      tower SE chain   0.9942  (se2-C256-G64-R1)
  stem                 0.9919  (C128, cin 128)         heads            0.2465  (C256, P32, V1, S1)
  pooled stats         0.1010  tower (se2-C256-G64-R3), 0.0932 stem (C256, cin 127)
Every x_out is stored in bf16, and its 2**-8 |ref| term IS the rounding of a value just above a power of two, so those ratios
sit just below 1; the fp32 outputs (pooled statistics, heads) stay below 0.25.  No kernel defect was found.
"""
import pytest
import torch

import tower_helpers as th
from conv_helpers import explain
from keisei_amd import _lib
from tower_helpers import F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
BF = torch.bfloat16
WORST = {}                                       # kernel -> (ratio, case): printed when the module is done
_PACKS, _TABLES = {}, {}


def st():
    return _lib.stream_ptr()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst error / bound per kernel")
    for k, (r, case) in sorted(WORST.items()):
        print(f"  {k:24s} {r:8.4f}  at {case}")
    _PACKS.clear(); _TABLES.clear()


def note(kernel, r, case):
    if r >= WORST.get(kernel, (-1.0, None))[0]:
        WORST[kernel] = (r, case)


def pack(w, kin):
    """ka_pack_conv3x3 mode 0 of w (Co, Ci, 3, 3) into Co x kin channels of bf16 fragments, once per weight tensor"""
    key = (id(w), kin)
    if key not in _PACKS:
        Co, Ci = w.shape[:2]
        wd = w.float().contiguous().to(DEV)
        buf = torch.zeros(th.pack_bytes(Co, kin), dtype=torch.uint8, device=DEV)
        _lib.call("ka_pack_conv3x3", wd, buf, Co, Ci, Co, kin, 0, _lib.DTYPE_BF16, st())
        torch.cuda.synchronize()
        _PACKS[key] = (buf, w)                   # (w kept: its id is the key)
    return _PACKS[key][0]


def tables(c, fields, kin=None):
    """the case's pointer table and the tensors behind it, kept for the life of the module"""
    if c.name not in _TABLES:
        _TABLES[c.name] = th.table(c.models, fields, DEV, pack, kin)
    return _TABLES[c.name][0]


def nans(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def mo_dev(model_of):
    return torch.tensor(list(model_of), dtype=torch.int32, device=DEV)


def run_tower(c, single=False, model_of=None, x=None, pool=None):
    """(x_out (B, 81, C) bf16, pool_out (B, 4C)) on the CPU, from NaN-filled buffers"""
    tab = tables(c, th.FIELDS)
    mo = c.model_of if model_of is None else model_of
    B = len(mo)
    xd = (c.x if x is None else x).to(BF).to(DEV).contiguous()
    pd = (c.pool_in if pool is None else pool).float().to(DEV).contiguous()
    xo, po = nans((B, th.BOARD, c.C), BF), nans((B, 4 * c.C))
    if single:
        assert c.K == 1 and all(m == 0 for m in mo)
        blocks = tab[0].contiguous()
        _lib.call("ka_tower_eval", xd, pd, xo, po, blocks, c.nb, B, c.C, c.G, c.R, _lib.DTYPE_BF16, st())
    else:
        _lib.call("ka_tower_eval_grouped", xd, pd, xo, po, mo_dev(mo), tab, c.K, c.nb, B, c.C, c.G, c.R, _lib.DTYPE_BF16, st())
    torch.cuda.synchronize()
    return xo.cpu(), po.cpu()


def run_stem(c, model_of=None):
    """obs sits at the front of a buffer whose remainder is NaN: exactly cin planes per board, a guard band behind the last"""
    tab = tables(c, th.STEM_FIELDS, th.STEM_KIN)
    mo = c.model_of if model_of is None else model_of
    n = c.obs.numel()
    buf = nans((n + 4 * th.BOARD,))
    buf[:n] = c.obs.float().reshape(-1).to(DEV)
    xo, po = nans((c.B, th.BOARD, c.C), BF), nans((c.B, 4 * c.C))
    _lib.call("ka_stem_eval_grouped", buf, mo_dev(mo), tab, c.K, xo, po, c.B, c.cin, c.C, _lib.DTYPE_BF16, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all())
    return xo.cpu(), po.cpu()


def assert_exact(c, xo, po, ref, what):
    C, B = c.C, xo.shape[0]
    assert torch.equal(xo.double(), ref["x"]), explain(f"{what} x_out", xo, ref["x"], B)
    assert torch.equal(po[:, C:2 * C].double(), ref["pool"][:, C:2 * C]), explain(f"{what} pooled max", po[:, C:2 * C], ref["pool"][:, C:2 * C], B)
    assert int(torch.count_nonzero(po[:, 3 * C:])) == 0 and bool(torch.isfinite(po).all()), f"{what}: the last quarter of pool_out"


def assert_pool(kernel, name, xo, po):
    r = th.judge_pool(xo, po)
    note(kernel, max(r["mean"], r["std"]), name)
    assert max(r.values()) <= 1.0, f"{name}: pool_out error / bound {r}"


# ------------------------------------------------------------------------------------------------ tier 1


@pytest.mark.parametrize("key", th.EXACT_TOWER, ids=lambda k: "-".join(map(str, k)))
def test_exact_tower(key):
    c, ref = th.exact_tower_case(*key), th.exact_tower_ref(*key)
    xo, po = run_tower(c)
    assert_exact(c, xo, po, ref, f"{c.name} grouped")
    if c.K == 1 and c.C == 256:
        assert _lib.query("ka_tower_eval_supported", c.C, c.G, c.R, _lib.DTYPE_BF16) == 1
        xs, ps = run_tower(c, single=True)
        assert_exact(c, xs, ps, ref, f"{c.name} ka_tower_eval")
        assert torch.equal(xs.view(torch.int16), xo.view(torch.int16)) and torch.equal(ps[:, :3 * c.C], po[:, :3 * c.C])


SEATS = (0, None, 1, 2, None, 3, 4)              # board of the 5-board case on each of 7 boards; None: unseated


@pytest.mark.parametrize("key", [k for k in th.EXACT_TOWER if k[4] == 5 and k[5] == 3], ids=lambda k: "-".join(map(str, k)))
def test_unseated_boards_of_the_tower_are_zero_and_disturb_nothing(key):
    c, ref = th.exact_tower_case(*key), th.exact_tower_ref(*key)
    full_x, full_p = run_tower(c)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 3, (7, th.BOARD, c.C), generator=g).float()
    pool = torch.randn(7, 4 * c.C, generator=g)
    mo = []
    for b, s in enumerate(SEATS):
        if s is None:
            mo.append(-1 if b == 1 else c.K)
        else:
            mo.append(c.model_of[s]); x[b] = c.x[s]; pool[b] = c.pool_in[s]
    xo, po = run_tower(c, model_of=mo, x=x, pool=pool)
    rows = [b for b, s in enumerate(SEATS) if s is not None]
    empty = [b for b, s in enumerate(SEATS) if s is None]
    assert int(torch.count_nonzero(xo[empty].view(torch.int16))) == 0 and int(torch.count_nonzero(po[empty].view(torch.int32))) == 0
    # G = 8 is the one width at which the row rotation (8 b) % G is the same on every board; elsewhere board b of this run and
    # board SEATS[b] of the full run walk the rows in another order, and must still agree to the bit: the operands are integers
    assert torch.equal(xo[rows].view(torch.int16), full_x.view(torch.int16)) and torch.equal(po[rows], full_p)
    assert torch.equal(xo[rows].double(), ref["x"])


@pytest.mark.parametrize("key", th.STEM_CASES, ids=lambda k: "-".join(map(str, k)))
def test_stem_exact(key):
    c = th.stem_case(*key)
    ref = th.stem_ref(c, F64)
    xo, po = run_stem(c)
    assert_exact(c, xo, po, ref, c.name)
    if c.K == 3:
        mo = tuple(-1 if b == 1 else c.K if b == 3 else m for b, m in enumerate(c.model_of))
        xu, pu = run_stem(c, model_of=mo)
        keep = [b for b in range(c.B) if b not in (1, 3)]
        assert int(torch.count_nonzero(xu[[1, 3]].view(torch.int16))) == 0 and int(torch.count_nonzero(pu[[1, 3]].view(torch.int32))) == 0
        assert torch.equal(xu[keep].view(torch.int16), xo[keep].view(torch.int16)) and torch.equal(pu[keep], po[keep])


# ------------------------------------------------------------------------------------------------ tier 2


@pytest.mark.parametrize("key", th.TIER2_GP, ids=lambda k: "-".join(map(str, k)))
def test_global_chain_tier2(key):
    c = th.tier2_case(*key)
    xo, po = run_tower(c)
    r = th.judge_x(xo, c)
    note("tower global chain", r, c.name)
    assert r <= 1.0, f"{c.name}: x_out error / bound {r}"
    assert torch.equal(xo, xo[:, :1].expand_as(xo)), "relu(g) must be the same on every square"
    assert_pool("pooled stats (tower)", c.name, xo, po)
    assert int(torch.count_nonzero(po[:, 2 * c.C:3 * c.C])) == 0, "every plane is constant: std exactly 0"


@pytest.mark.parametrize("key", th.TIER2_SE, ids=lambda k: "-".join(map(str, k)))
def test_se_chain_tier2(key):
    c = th.tier2_case(*key)
    xo, po = run_tower(c)
    r = th.judge_x(xo, c)
    note("tower SE chain", r, c.name)
    assert r <= 1.0, f"{c.name}: x_out error / bound {r}"
    assert_pool("pooled stats (tower)", c.name, xo, po)
    C = c.C
    assert float(po[:, 2 * C + 5].abs().max()) == 0 and float(po[:, C + 5].min()) > 0, "the constant plane"
    assert float(po[:, [9, C + 9, 2 * C + 9]].abs().max()) == 0, "the all-zero plane"
    assert torch.equal(po[:, C + 14], xo[:, 80, 14].float()), "the maximum on square 80"


@pytest.mark.parametrize("key", th.STEM_CASES, ids=lambda k: "-".join(map(str, k)))
def test_stem_affine_tier2(key):
    c = th.stem_case(*key, real=True)
    xo, po = run_stem(c)
    r = th.judge_x(xo, c, lambda c, dt: th.stem_ref(c, dt)["pre"])
    note("stem", r, c.name)
    assert r <= 1.0, f"{c.name}: x_out error / bound {r}"
    assert_pool("pooled stats (stem)", c.name, xo, po)
    C = c.C
    assert float(po[:, 2 * C + 5].abs().max()) == 0 and float(po[:, C + 5].min()) > 0, "the constant plane"
    assert float(po[:, [9, C + 9, 2 * C + 9]].abs().max()) == 0, "the all-zero plane"


@pytest.mark.parametrize("key", th.HEADS_CASES, ids=lambda k: "-".join(map(str, k)))
def test_heads(key):
    c = th.heads_case(*key)
    tab = tables(c, th.HEAD_FIELDS)
    B = c.B
    x, pool = c.x.to(BF).to(DEV).contiguous(), c.pool.float().to(DEV).contiguous()
    got = {"logits": nans((B, 9, 9, th.MOVES)), "value": nans((B, 3)), "score": nans((B, 1))}
    _lib.call("ka_heads_eval_grouped", x, pool, mo_dev(c.model_of), tab, c.K, got["logits"], got["value"], got["score"], B, c.C, c.P,
              c.V, c.S, _lib.DTYPE_BF16, st())
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in got.items()}
    r = th.judge_heads(got, c)
    note("heads", max(r.values()), c.name)
    assert max(r.values()) <= 1.0, f"{c.name}: error / bound {r}"
    empty = [b for b, m in enumerate(c.model_of) if not th.seated(m, c.K)]
    assert len(empty) == 2
    for v in got.values():
        assert int(torch.count_nonzero(v[empty].view(torch.int32))) == 0
    # the layout: a move-major store of the same numbers is far outside the bound (test_tower_oracle_cpu.py); the logits of a
    # square differ from move to move
    assert float(got["logits"][0].reshape(th.BOARD, th.MOVES).std(1).min()) > 0
