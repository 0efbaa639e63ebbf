"""Shared by tests/test_tower_oracle_cpu.py and tests/test_hip_tower_oracle.py: the cases, the float64 references, the mutants
and the pointer tables of the eval tower, the grouped stem and the grouped heads (csrc/tower.hip).  No GPU in here: the table
builders take the device and a packing function from the caller.

References.  `tower_ref`, `stem_ref` and `heads_ref` are written from the model (oracle/keisei_oracle.py block_forward /
seresnet_forward) with BatchNorm folded into (scale, shift), and round to bf16 exactly where tower.hip does (rnd=True): the
conv outputs y0 / y1 / y2 as the epilogues read them, h = relu(bn1 y1) + g, and every block output.  With rnd=False in float64
they ARE the model (test_tower_oracle_cpu.py proves it at shapes outside the two the end-to-end tests use).

Tier 1 (exact).  Operands are small integers, so every product and every fp32 partial sum is exact in any order and every
stored bf16 is an integer <= 256: the kernel must equal the float64 reference to the bit.  The inexact steps of the FC chains
are routed around (see exact_tower_case); `check_exact_tower` / `check_exact_stem` assert the conditions on the reference.
  "conv" cases: both convolutions non-zero, the global chain live through the max columns, the SE transparent (sw2 = 0,
                gate bias 40, an integer shift per channel);
  "se"   cases: w2 = 0, so z = sh2 (even) and the squeeze is sh2 exactly; gate rows in {0, 40}: every gate is 0.5 or 1.
Tier 2 (float64 oracle, one rounding per output).  Real-valued operands; the convolutions are exact pass-throughs so that the
compared value goes through ONE bf16 rounding, and is held to board_helpers.bound_of (MARGIN x e32 + 2**-8 |ref|).
  "gp"   cases: x_in = 0, w2 = centre-tap identity, SE transparent: x_out[b, p, c] = bf16(relu(g[b, c])), g the real-valued
                global chain over a pool_in of the test's choosing (all three column groups live);
  "se2"  cases: w1 = w2 = centre-tap identity, g = 0: y2 = x exactly, x_out = bf16(relu((sc2 x + sh2) sigmoid(s[:C]) + s[C:] + x)).
pool_out is held to the statistics of the kernel's OWN x_out (`judge_pool`); the heads have no internal rounding and are held
to `heads_ref` directly.

Mutants: every reference takes `mutant=`, one wrong line each (MUTANTS)."""
import functools
import math
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from board_helpers import ratio                                  # error / (MARGIN x e32 [+ 2**-8 |ref| for bf16]): board_helpers.bound_of
from conv_helpers import BF16_INT, LIMIT, amax, gen, ints, nchw, nhwc, pick, sparse_ternary
from update_head_helpers import FLOOR, MARGIN, e32_of          # noqa: F401  (the bound is the project's own)

BOARD, MOVES = 81, 139
F64, F32 = torch.float64, torch.float32
STEM_KIN = 128
FIELDS = ("w1", "w2", "sc1", "sh1", "sc2", "sh2", "gw1", "gb1", "gw2", "gb2", "sw1", "sb1", "sw2", "sb2")      # TowerBlock
STEM_FIELDS = ("w", "sc", "sh")                                                                                  # StemRow
HEAD_FIELDS = ("wp1", "scp", "shp", "wp2", "bp2", "v1w", "v1b", "v2w", "v2b", "s1w", "s1b", "s2w", "s2b")        # HeadRow
GS, RS = (8, 24, 72, 200, 256), (1, 3, 16, 36, 64)
CINS = (1, 46, 50, 127, 128)
MUTANTS = ("tap8_last_kstep", "max_no_sq80", "std_corr1", "rot_not_bias", "se_last_row", "se_halves_swapped", "prev_board_g",
           "next_model", "move_major", "stem_plane_cin")


def qb(t: torch.Tensor) -> torch.Tensor:
    """round to bf16, keep the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def ident(t):
    return t


def is_bf16(t: torch.Tensor) -> bool:
    return torch.equal(t, qb(t))


def halves(t: torch.Tensor) -> bool:
    """every element an integer or a half"""
    return bool(((2 * t) == (2 * t).round()).all())


def seated(m: int, K: int) -> bool:
    return 0 <= m < K


# ------------------------------------------------------------------------------------------------ the references


def conv3(x, w, dt, mutant=None, kin=None):
    """3x3 convolution, padding 1: x (n, 81, Ci), w (Co, Ci, 3, 3) -> (n, 81, Co).  mutant tap8_last_kstep: the kernel's last
    k-step (input channels kin - 32 .. kin - 1 of tap 8) is dropped."""
    w = w.to(dt)
    if mutant == "tap8_last_kstep":
        kin = kin or w.shape[1]
        w = w.clone()
        w[:, kin - 32:kin, 2, 2] = 0
    return nhwc(F.conv2d(nchw(x.to(dt)), w, padding=1))


def pool3(x, dt, mutant=None):
    """[mean | max | population std] of (n, 81, C) -> (n, 3C)            (keisei_oracle.global_pool)"""
    x = x.to(dt)
    mean = x.sum(1) / BOARD
    mx = (x[:, :80] if mutant == "max_no_sq80" else x).amax(1)
    var = ((x - mean[:, None]) ** 2).sum(1) / (BOARD - 1 if mutant == "std_corr1" else BOARD)
    return torch.cat([mean, mx, var.sqrt()], 1)


def gchain(wb, p3, dt, mutant=None, rot=0, tr=None):
    """g = W2 relu(W1 [mean|max|std] + b1) + b2 of one board, p3 (1, 3C).  rot: the kernel's row rotation (8 b) % G, which
    must not show; mutant rot_not_bias: row (j + rot) % G takes the bias of row j."""
    b1 = wb["gb1"].to(dt)
    if mutant == "rot_not_bias":
        b1 = b1.roll(rot)
    hid = torch.relu(p3.to(dt) @ wb["gw1"].to(dt).t() + b1)
    g = hid @ wb["gw2"].to(dt).t() + wb["gb2"].to(dt)
    if tr is not None:
        tr["fc"] = max(tr.get("fc", 0.0), _fcmax(p3, wb["gw1"], wb["gb1"]), _fcmax(hid, wb["gw2"], wb["gb2"]))
    return g


def _fcmax(v, w, b):
    """the largest sum of magnitudes of an FC layer: no partial sum, in any order, is larger"""
    return amax(v.double().abs() @ w.double().abs().t() + b.double().abs())


def block_rest(wb, x, g, dt, rnd, mutant=None, tr=None):
    """everything of a block behind g, on one board: x (1, 81, C), g (1, C) -> dict(out, pre, ...)"""
    q = qb if rnd else ident
    C = x.shape[2]
    W = {k: wb[k].to(dt) for k in FIELDS[2:]}
    y1 = conv3(x, wb["w1"], dt, mutant)
    h = q(torch.relu(q(y1) * W["sc1"] + W["sh1"]) + g[:, None])
    y2 = conv3(h, wb["w2"], dt, mutant)
    sq = y2.sum(1) / BOARD * W["sc2"] + W["sh2"]                    # the squeeze takes the unrounded conv output
    z = q(y2) * W["sc2"] + W["sh2"]
    w1, b1 = W["sw1"], W["sb1"]
    e1 = torch.relu(sq @ w1.t() + b1)
    if mutant == "se_last_row":
        e1 = e1.clone()
        e1[:, -1] = 0
    s = e1 @ W["sw2"].t() + W["sb2"]
    if mutant == "se_halves_swapped":
        s = torch.cat([s[:, C:], s[:, :C]], 1)
    pre = torch.relu(z * torch.sigmoid(s[:, None, :C]) + s[:, None, C:] + x.to(dt))
    r = {"y1": y1, "h": h, "y2": y2, "sq": sq, "z": z, "e1": e1, "s": s, "pre": pre, "out": q(pre), "g": g}
    if tr is not None:
        tr["fc"] = max(tr.get("fc", 0.0), _fcmax(sq, wb["sw1"], wb["sb1"]), _fcmax(e1, wb["sw2"], wb["sb2"]))
    return r


class Tower(NamedTuple):
    name: str
    kind: str                                    # conv | se (exact), gp | se2 (tier 2), model (real weights, no structure)
    C: int
    G: int
    R: int
    nb: int
    K: int
    model_of: Tuple[int, ...]
    models: tuple                                # [K][nb] dicts of FIELDS -> float32 (or float64) CPU tensors
    x: torch.Tensor                              # (B, 81, C), bf16-exact values
    pool_in: torch.Tensor                        # (B, 4C)

    @property
    def B(self):
        return len(self.model_of)


def tower_ref(c: Tower, dt, rnd=True, mutant=None, model_of=None, trace=False) -> dict:
    """x (B, 81, C) as stored, pre (the last block's output before its rounding), pool (B, 4C) = [mean|max|std|0] of x, and
    trace = one dict per block of (B, ...) tensors.  Unseated boards: zeros.  Block 0 takes the case's pool_in, the later ones
    the statistics of the previous output (mutants max_no_sq80 / std_corr1 apply there and to `pool`)."""
    mo = list(c.model_of if model_of is None else model_of)
    B, C, K = len(mo), c.C, c.K
    rows = [b for b in range(B) if seated(mo[b], K)]
    mdl = {b: ((mo[b] + 1) % K if mutant == "next_model" else mo[b]) for b in rows}
    x = {b: c.x[b:b + 1].to(dt) for b in rows}
    p3 = {b: c.pool_in[b:b + 1, :3 * C].to(dt) for b in rows}
    traces, last = [], {}
    for i in range(c.nb):
        tr = {} if trace else None
        g = {b: gchain(c.models[mdl[b]][i], p3[b], dt, mutant, (8 * b) % c.G, tr) for b in rows}
        if mutant == "prev_board_g":
            g = {b: g[rows[(k - 1) % len(rows)]] for k, b in enumerate(rows)}
        last = {b: block_rest(c.models[mdl[b]][i], x[b], g[b], dt, rnd, mutant, tr) for b in rows}
        x = {b: last[b]["out"] for b in rows}
        p3 = {b: pool3(x[b], dt, mutant) for b in rows}
        if trace:
            tr.update({k: torch.cat([last[b][k] for b in rows]) for k in last[rows[0]]})
            tr["pool"] = torch.cat([p3[b] for b in rows])
            traces.append(tr)
    out = {"x": torch.zeros(B, BOARD, C, dtype=dt), "pre": torch.zeros(B, BOARD, C, dtype=dt), "pool": torch.zeros(B, 4 * C, dtype=dt)}
    for b in rows:
        out["x"][b], out["pre"][b], out["pool"][b, :3 * C] = x[b][0], last[b]["pre"][0], p3[b][0]
    out["trace"], out["rows"] = traces, rows
    return out


class Stem(NamedTuple):
    name: str
    C: int
    cin: int
    K: int
    model_of: Tuple[int, ...]
    models: tuple                                # [K] dicts of STEM_FIELDS (w: (C, cin, 3, 3))
    obs: torch.Tensor                            # (B, cin, 9, 9), bf16-exact

    @property
    def B(self):
        return len(self.model_of)


def stem_ref(c: Stem, dt, rnd=True, mutant=None) -> dict:
    """x = relu(input_bn(input_conv(obs))) (B, 81, C) as stored, pre, pool.  mutant stem_plane_cin: the kernel reads one plane
    too many -- plane cin is the next board's plane 0, or the NaN guard band behind the last board -- against the zero weights
    the pack holds past cin (0 x NaN is a NaN); it cannot happen at cin = 128, the width of the staging chunk."""
    q = qb if rnd else ident
    B, K, cin = c.B, c.K, c.cin
    out = {"x": torch.zeros(B, BOARD, c.C, dtype=dt), "pre": torch.zeros(B, BOARD, c.C, dtype=dt), "pool": torch.zeros(B, 4 * c.C, dtype=dt),
           "y": torch.zeros(B, BOARD, c.C, dtype=dt)}
    obs = c.obs.to(dt)
    if mutant == "stem_plane_cin" and cin < STEM_KIN:
        flat = torch.cat([obs.reshape(-1), torch.full((BOARD,), float("nan"), dtype=dt)])
        extra = torch.stack([flat[(b * cin + cin) * BOARD:(b * cin + cin + 1) * BOARD] for b in range(B)]).reshape(B, 1, 9, 9)
        obs = torch.cat([obs, extra], 1)
    for b in range(B):
        m = c.model_of[b]
        if not seated(m, K):
            continue
        sw = c.models[(m + 1) % K if mutant == "next_model" else m]
        w = sw["w"].to(dt)
        if obs.shape[1] > cin:
            w = torch.cat([w, torch.zeros(c.C, 1, 3, 3, dtype=dt)], 1)
        y = conv3(nhwc(q(obs[b:b + 1])), w, dt, mutant, kin=STEM_KIN)
        pre = torch.relu(q(y) * sw["sc"].to(dt) + sw["sh"].to(dt))
        out["y"][b], out["pre"][b], out["x"][b] = y[0], pre[0], q(pre)[0]
        out["pool"][b, :3 * c.C] = pool3(out["x"][b:b + 1], dt, mutant)[0]
    return out


class Heads(NamedTuple):
    name: str
    C: int
    P: int
    V: int
    S: int
    K: int
    model_of: Tuple[int, ...]
    models: tuple                                # [K] dicts of HEAD_FIELDS
    x: torch.Tensor                              # (B, 81, C) bf16-exact
    pool: torch.Tensor                           # (B, 4C): an input of its own, the last quarter never read

    @property
    def B(self):
        return len(self.model_of)


def heads_ref(c: Heads, dt, mutant=None) -> dict:
    """logits (B, 9, 9, 139) = policy_conv2(relu(policy_bn1(policy_conv1(x)))) with the move index fastest, value (B, 3),
    score (B, 1) over [mean|max|std]; zeros for an unseated board.  mutant move_major: logits stored (139, 81) per board."""
    B, C = c.B, c.C
    out = {"logits": torch.zeros(B, 9, 9, MOVES, dtype=dt), "value": torch.zeros(B, 3, dtype=dt), "score": torch.zeros(B, 1, dtype=dt)}
    for b in range(B):
        m = c.model_of[b]
        if not seated(m, c.K):
            continue
        W = {k: v.to(dt) for k, v in c.models[(m + 1) % c.K if mutant == "next_model" else m].items()}
        p1 = torch.relu((c.x[b].to(dt) @ W["wp1"].t()) * W["scp"] + W["shp"])                 # (81, P)
        lg = p1 @ W["wp2"].t() + W["bp2"]                                                     # (81, 139)
        out["logits"][b] = (lg.t().contiguous() if mutant == "move_major" else lg).reshape(9, 9, MOVES)
        p = c.pool[b, :3 * C].to(dt)
        out["value"][b] = torch.relu(p @ W["v1w"].t() + W["v1b"]) @ W["v2w"].t() + W["v2b"]
        out["score"][b] = torch.relu(p @ W["s1w"].t() + W["s1b"]) @ W["s2w"].t() + W["s2b"]
    return out


# ------------------------------------------------------------------------------------------------ judging


def judge_x(got, c, fn=None) -> float:
    """a tier-2 x_out (B, 81, C) as stored in bf16 against the float64 value it is ONE rounding of: error / bound"""
    fn = fn or expect
    r64, r32 = fn(c, F64), fn(c, F32)
    return ratio(got, r64, e32_of(r32.double(), r64), torch.bfloat16)


def judge_pool(xs: torch.Tensor, pool: torch.Tensor, mutant=None) -> dict:
    """pool (B, 4C) against the statistics of the stored xs (B, 81, C): mean and std within the fp32 bound, max equal, the
    last quarter zero, and std exactly 0 on every constant plane (inf where an exact condition fails)"""
    xs, pool = xs.detach().double().cpu(), pool.detach().double().cpu()
    C = xs.shape[2]
    r64, r32 = pool3(xs, F64), pool3(xs, F32).double()
    out = {}
    for k, name in enumerate(("mean", "max", "std")):
        a, b, got = r64[:, k * C:(k + 1) * C], r32[:, k * C:(k + 1) * C], pool[:, k * C:(k + 1) * C]
        out[name] = (0.0 if torch.equal(got, a) else math.inf) if name == "max" else ratio(got, a, e32_of(b, a))
    const = xs.amax(1) == xs.amin(1)
    if not torch.equal(pool[:, 2 * C:3 * C][const], torch.zeros(int(const.sum()), dtype=F64)):
        out["std"] = math.inf
    out["zero"] = 0.0 if int(torch.count_nonzero(pool[:, 3 * C:])) == 0 else math.inf
    return out


def judge_heads(got: dict, c: Heads) -> dict:
    r64, r32 = heads_ref(c, F64), heads_ref(c, F32)
    return {k: ratio(got[k], r64[k], e32_of(r32[k].double(), r64[k])) for k in ("logits", "value", "score")}


def stored_pool(p: torch.Tensor) -> torch.Tensor:
    return p.float().double()


# ------------------------------------------------------------------------------------------------ tier 1: the exact cases

MIXED = {(1, 1): (0,), (1, 3): (1,), (5, 1): (0,) * 5, (5, 3): (2, 0, 1, 0, 2)}


def _sparse_rows(g, n, rows, cols, values=(-1.0, 1.0)):
    """about n non-zero entries per row"""
    keep = torch.rand(rows, cols, generator=g) < min(1.0, n / cols)
    return pick(g, values, rows, cols) * keep


def exact_block(g, kind, C, G, R, n1, n2, gn):
    """One block of integer weights (module docstring).  n1 / n2: non-zero taps per output channel of conv1 / conv2; gn:
    non-zero max columns per row of global_fc[0], 0 = one +1 and one -1 (the difference of two maxima: the later blocks, whose
    maxima are large)."""
    wb = {"w1": sparse_ternary(g, n1, 9 * C, C, C, 3, 3), "w2": sparse_ternary(g, n2, 9 * C, C, C, 3, 3)}
    wb["sc1"], wb["sh1"] = pick(g, (1.0, 1.0, 1.0, 2.0), C), ints(g, 1, C)
    wb["sc2"], wb["sh2"] = pick(g, (1.0, 1.0, 1.0, 2.0), C), ints(g, 1, C)
    gw1 = torch.zeros(G, 3 * C)
    if gn:                                                          # mean and std columns: zero weights
        gw1[:, C:2 * C] = _sparse_rows(g, gn, G, C)
    else:
        rows = torch.arange(G)
        gw1[rows, C + torch.randint(0, C, (G,), generator=g)] += 1.0
        gw1[rows, C + torch.randint(0, C, (G,), generator=g)] -= 1.0
    wb["gw1"], wb["gb1"] = gw1, ints(g, 2, G)
    wb["gw2"], wb["gb2"] = _sparse_rows(g, 1.5 if gn else 0.5, C, G), ints(g, 1, C)
    wb["sw1"], wb["sb1"] = _sparse_rows(g, 4, R, C), ints(g, 2, R)
    if kind == "conv":                                              # transparent SE: gate logit 40 whatever e1, an integer shift
        wb["sw2"] = torch.zeros(2 * C, R)
        wb["sb2"] = torch.cat([torch.full((C,), 40.0), ints(g, 1, C)])
    else:                                                           # w2 = 0: z = sh2, even where the gate is 0.5
        wb["w2"] = torch.zeros(C, C, 3, 3)
        wb["sh2"] = 2 * ints(g, 1, C)
        wb["sb1"][R - 1] = 2.0 + 2.0 * float(wb["sw1"][R - 1].abs().sum())      # the last hidden unit is alive on every board
        gate = _sparse_rows(g, min(1.5, 0.5 * R), C, R, (40.0,))
        wb["sw2"] = torch.cat([gate, _sparse_rows(g, 3, C, R)])
        wb["sb2"] = torch.cat([torch.zeros(C), ints(g, 1, C)])
    return wb


@functools.lru_cache(maxsize=None)
def exact_tower_case(kind, C, G, R, B, K, nb) -> Tower:
    """x_in: integers in {0, 1, 2}; pool_in: the true max of x_in, garbage-but-finite mean / std / last quarter (they meet
    zero weights only).  Every model gets its own weights.  Later blocks are sparser: the activations grow block by block and
    every stored value must stay an integer <= 256."""
    g = gen(11, kind == "se", C, G, R, B, K, nb)
    dense = (16, 8, 16) if nb == 1 else (2, 1, 4)
    models = tuple(tuple(exact_block(g, kind, C, G, R, *(dense if i == 0 else (0.25, 0.25, 0))) for i in range(nb)) for _ in range(K))
    x = pick(g, (0.0, 0.0, 1.0, 2.0), B, BOARD, C)
    pool = 1000.0 * torch.randn(B, 4 * C, generator=g)
    pool[:, C:2 * C] = x.amax(1)
    return Tower(f"{kind}-C{C}-G{G}-R{R}-B{B}-K{K}-nb{nb}", kind, C, G, R, nb, K, MIXED[(B, K)], models, x, pool)


# (G, R, B, K, nblocks) per channel count: every G and every R at both C in both families, B in {1, 5}, K in {1, 3} mixed
_SHAPES = ((8, 16, 5, 3, 1), (24, 3, 1, 1, 3), (72, 36, 5, 1, 3), (200, 1, 5, 3, 3), (256, 64, 1, 3, 1))
_SHAPES_SE = ((8, 3, 1, 3, 3), (24, 64, 5, 3, 1), (72, 1, 5, 1, 1), (200, 16, 1, 1, 1), (256, 36, 5, 3, 3))
EXACT_TOWER = tuple(("conv", C, *s) for C in (128, 256) for s in _SHAPES) + tuple(("se", C, *s) for C in (128, 256) for s in _SHAPES_SE)


@functools.lru_cache(maxsize=None)
def exact_tower_ref(*key) -> dict:
    return tower_ref(exact_tower_case(*key), F64, trace=True)


def check_exact_tower(c: Tower, ref: Optional[dict] = None) -> dict:
    """The conditions under which the kernel must equal the float64 reference to the bit, asserted on that reference; returns
    what was seen (largest stored value, the gate values)."""
    ref = ref or tower_ref(c, F64, trace=True)
    C = c.C
    assert bool(torch.isfinite(c.pool_in).all()) and is_bf16(c.x) and halves(c.x) and float(c.x.min()) >= 0
    assert torch.equal(c.pool_in[:, C:2 * C].double(), c.x.double().amax(1)), "block 0 must be given the true max"
    for blocks in c.models:
        for wb in blocks:
            assert amax(wb["gw1"][:, :C]) == 0 and amax(wb["gw1"][:, 2 * C:]) == 0, "mean / std columns must be zero"
            assert all(halves(wb[k]) for k in FIELDS) and is_bf16(wb["w1"]) and is_bf16(wb["w2"])
            assert amax(wb["w1"]) <= 1 and amax(wb["w2"]) <= 1
            gate_w, gate_b = wb["sw2"][:C], wb["sb2"][:C]
            assert bool(((gate_w == 0) | (gate_w == 40)).all()) and bool(((gate_b == 0) | (gate_b == 40)).all())
    top, gates = 0.0, set()
    xin = c.x.double()[ref["rows"]]
    for tr in ref["trace"]:
        live = ("y1", "h", "y2", "z", "g", "pre", "out") + (("sq", "e1", "s") if c.kind == "se" else ())
        for k in live:
            assert halves(tr[k]), f"{c.name}: {k} is not made of integers and halves"
        for k in ("y1", "h", "y2", "out"):
            assert is_bf16(tr[k]) and amax(tr[k]) <= BF16_INT, f"{c.name}: {k} is not stored exactly as bf16 (max {amax(tr[k])})"
            top = max(top, amax(tr[k]))
        assert 9 * C * amax(xin) < LIMIT and 9 * C * amax(tr["h"]) < LIMIT, f"{c.name}: a conv partial sum could reach 2^24"
        assert BOARD * max(amax(tr["y2"]), amax(tr["out"])) < LIMIT
        assert tr["fc"] < LIMIT, f"{c.name}: an FC partial sum could reach 2^24"
        logit = tr["s"][:, :C]
        assert bool(((logit == 0) | (logit >= 40)).all()), f"{c.name}: a gate logit in (0, 40)"
        gates |= set(torch.sigmoid(logit).unique().tolist())
        if c.kind == "se":
            assert amax(tr["y2"]) == 0 and bool((tr["z"] % 2 == 0).all())
        assert torch.equal(tr["pool"][:, C:2 * C], tr["out"].amax(1))
        xin = tr["out"]
    assert gates <= {0.5, 1.0}
    return {"top": top, "gates": gates}


# ------------------------------------------------------------------------------------------------ the stem cases


@functools.lru_cache(maxsize=None)
def stem_case(C, cin, B, K, real=False) -> Stem:
    """obs in {-1, 0, 1, 2}, ternary weights of density 1/4; input_bn scale in {1, 2} and shift in {-1, 0, 1} (exact), or real
    (tier 2: the conv is still exact, x_out one rounding of y sc + sh); channel 5 has no weights (a constant plane: std exactly
    0), channel 9 none and a negative shift (an all-zero plane)."""
    g = gen(12, C, cin, B, K, real)
    models = []
    for _ in range(K):
        w = sparse_ternary(g, 1, 4, C, cin, 3, 3)
        if real:
            sc, sh = (torch.rand(C, generator=g) + 0.5), torch.randn(C, generator=g)
            w[5], w[9] = 0, 0
            sh[5], sh[9] = 0.7, -1.0
        else:
            sc, sh = pick(g, (1.0, 2.0), C), ints(g, 1, C)
        models.append({"w": w, "sc": sc, "sh": sh})
    obs = pick(g, (-1.0, 0.0, 1.0, 2.0), B, cin, 9, 9)
    mo = MIXED[(B, K)] if (B, K) in MIXED else tuple((3 * b + 1) % K for b in range(B))
    return Stem(f"stem-C{C}-cin{cin}-B{B}-K{K}" + ("-real" if real else ""), C, cin, K, mo, tuple(models), obs)


STEM_CASES = tuple((C, cin, 5, 3) for C in (128, 256) for cin in CINS) + ((256, 46, 1, 1), (128, 50, 1, 1))


def check_exact_stem(c: Stem, ref=None, real=False):
    """exact case: everything an integer <= 256; tier 2: the conv output is an exactly stored integer (one rounding follows)"""
    ref = ref or stem_ref(c, F64)
    assert is_bf16(c.obs) and halves(c.obs) and all(is_bf16(m["w"]) for m in c.models)
    assert 9 * STEM_KIN * amax(c.obs) < LIMIT
    assert halves(ref["y"]) and is_bf16(ref["y"]) and amax(ref["y"]) <= BF16_INT
    if not real:
        assert halves(ref["pre"]) and amax(ref["pre"]) <= BF16_INT and torch.equal(ref["pre"], ref["x"])
        assert BOARD * amax(ref["x"]) < LIMIT


# ------------------------------------------------------------------------------------------------ tier 2


def centre_identity(C):
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return w


def _f32(t):
    return t.float()


@functools.lru_cache(maxsize=None)
def tier2_case(kind, C, G, R, B=5, K=3) -> Tower:
    g = gen(13, kind == "se2", C, G, R, B, K)
    rn = lambda *s: torch.randn(*s, generator=g)
    eye, models = centre_identity(C), []
    for _ in range(K):
        wb = {"w1": eye, "w2": eye, "sc1": torch.ones(C), "sh1": torch.zeros(C)}
        wb["sw1"], wb["sb1"] = rn(R, C) / C ** 0.5, 0.5 * rn(R)
        wb["sb1"][R - 1] = 2.0                                      # the last hidden unit is alive
        if kind == "gp":
            wb["sc2"], wb["sh2"] = torch.ones(C), torch.zeros(C)
            wb["gw1"], wb["gb1"] = rn(G, 3 * C) / (3 * C) ** 0.5, 0.5 * rn(G)
            wb["gw2"], wb["gb2"] = rn(C, G) / G ** 0.5, 0.3 * rn(C)
            wb["sw2"], wb["sb2"] = torch.zeros(2 * C, R), torch.cat([torch.full((C,), 40.0), torch.zeros(C)])
        else:
            wb["sc2"], wb["sh2"] = torch.rand(C, generator=g) + 0.5, 0.3 * rn(C)
            wb["gw1"], wb["gb1"] = rn(G, 3 * C) / (3 * C) ** 0.5, 0.5 * rn(G)
            wb["gw2"], wb["gb2"] = torch.zeros(C, G), torch.zeros(C)
            wb["sw2"], wb["sb2"] = rn(2 * C, R) / R ** 0.5, rn(2 * C)
            # channel 9: gate 0.5, shift -1, sh2 -1 on an all-zero input plane: an all-zero output plane
            wb["sw2"][9], wb["sw2"][C + 9], wb["sb2"][9], wb["sb2"][C + 9], wb["sh2"][9] = 0, 0, 0.0, -1.0, -1.0
            for ch in (5, 14):                                      # the constant plane and the one with its max on square 80 stay positive
                wb["sw2"][C + ch], wb["sb2"][C + ch], wb["sh2"][ch] = 0, 0.25, 0.1
        models.append((wb,))
    if kind == "gp":
        x = torch.zeros(B, BOARD, C)
        pool = torch.cat([rn(B, C).abs(), 1.0 + rn(B, C).abs(), rn(B, C).abs(), rn(B, C)], 1)
    else:
        x = qb(torch.relu(rn(B, BOARD, C)))
        x[:, :, 5], x[:, :, 9] = 0.75, 0.0                          # a constant plane, an all-zero plane
        x[:, :, 14] = qb(torch.rand(B, BOARD, generator=g))
        x[:, 80, 14] = 1.5                                          # the maximum on square 80 alone
        pool = torch.cat([pool3(x, F64).float(), rn(B, C)], 1)
    mo = MIXED[(B, K)] if (B, K) in MIXED else tuple(b % K for b in range(B))
    return Tower(f"{kind}-C{C}-G{G}-R{R}", kind, C, G, R, 1, K, mo, tuple(models), x, pool)


TIER2_GP = tuple(("gp", C, G, 16) for C in (128, 256) for G in GS)
TIER2_SE = tuple(("se2", C, 64, R) for C in (128, 256) for R in RS)


def expect(c: Tower, dt, mutant=None) -> torch.Tensor:
    """the value x_out is one bf16 rounding of: relu(g) on every square (gp), the block formula over y2 = x (se2)"""
    r = tower_ref(c, dt, mutant=mutant, trace=True)
    if c.kind != "gp":
        return r["pre"]
    out = torch.zeros(c.B, BOARD, c.C, dtype=dt)
    out[r["rows"]] = torch.relu(r["trace"][0]["g"])[:, None].expand(-1, BOARD, -1)
    return out


def check_single_rounding(c: Tower) -> None:
    """the intermediate a pass-through is meant to carry equals its source exactly, in float64 and in float32"""
    for dt in (F64, F32):
        r = tower_ref(c, dt, trace=True)
        tr, rows = r["trace"][0], r["rows"]
        if c.kind == "gp":
            assert amax(c.x) == 0 and amax(tr["y1"]) == 0
            assert torch.equal(tr["h"], qb(tr["g"])[:, None].expand(-1, BOARD, -1)) and torch.equal(tr["y2"], tr["h"])
            assert torch.equal(tr["z"], tr["h"]) and bool((torch.sigmoid(tr["s"][:, :c.C]) == 1).all()) and amax(tr["s"][:, c.C:]) == 0
            assert torch.equal(r["x"], qb(expect(c, dt)))
        else:
            assert amax(tr["g"]) == 0 and is_bf16(c.x) and float(c.x.min()) >= 0
            assert torch.equal(tr["y1"], c.x.to(dt)[rows]) and torch.equal(tr["h"], tr["y1"]) and torch.equal(tr["y2"], tr["h"])
            assert torch.equal(r["x"], qb(r["pre"]))


@functools.lru_cache(maxsize=None)
def heads_case(C, P, V, S, B=7, K=3) -> Heads:
    """real-valued everything; boards 1 and 4 unseated (model -1 and K)"""
    g = gen(14, C, P, V, S, B, K)
    rn = lambda *s: torch.randn(*s, generator=g)
    models = []
    for _ in range(K):
        models.append({"wp1": rn(P, C) / C ** 0.5, "scp": torch.rand(P, generator=g) + 0.5, "shp": 0.3 * rn(P),
                       "wp2": rn(MOVES, P) / P ** 0.5, "bp2": 0.3 * rn(MOVES),
                       "v1w": rn(V, 3 * C) / (3 * C) ** 0.5, "v1b": 0.3 * rn(V), "v2w": rn(3, V) / V ** 0.5, "v2b": 0.3 * rn(3),
                       "s1w": rn(S, 3 * C) / (3 * C) ** 0.5, "s1b": 0.3 * rn(S), "s2w": rn(1, S) / S ** 0.5, "s2b": 0.3 * rn(1)})
    x = qb(torch.relu(rn(B, BOARD, C)))
    pool = torch.cat([rn(B, 3 * C), 1000.0 * rn(B, C)], 1)
    mo = (2, -1, 0, 1, K, 1, 0)[:B]
    return Heads(f"heads-C{C}-P{P}-V{V}-S{S}", C, P, V, S, K, mo, tuple(models), x, pool)


HEADS_CASES = tuple((C, P, V, S) for C in (128, 256) for P in (1, 7, 32) for V, S in ((1, 1), (3, 65), (200, 130), (512, 512)))


# ------------------------------------------------------------------------------------------------ the model as a case


def fold_bn(sd, prefix, eps=1e-5):
    sc = sd[prefix + ".weight"] / torch.sqrt(sd[prefix + ".running_var"] + eps)
    return sc, sd[prefix + ".bias"] - sd[prefix + ".running_mean"] * sc


def model_parts(sd, shape):
    """(stem row, tower blocks, head row) of a state_dict, BatchNorm folded, in the dtype of sd"""
    sc, sh = fold_bn(sd, "input_bn")
    stem = {"w": sd["input_conv.weight"], "sc": sc, "sh": sh}
    blocks = []
    for i in range(shape.num_blocks):
        p = f"blocks.{i}."
        wb = {"w1": sd[p + "conv1.weight"], "w2": sd[p + "conv2.weight"]}
        wb["sc1"], wb["sh1"] = fold_bn(sd, p + "bn1")
        wb["sc2"], wb["sh2"] = fold_bn(sd, p + "bn2")
        for k, n in (("gw1", "global_fc.0.weight"), ("gb1", "global_fc.0.bias"), ("gw2", "global_fc.2.weight"), ("gb2", "global_fc.2.bias"),
                     ("sw1", "se_fc1.weight"), ("sb1", "se_fc1.bias"), ("sw2", "se_fc2.weight"), ("sb2", "se_fc2.bias")):
            wb[k] = sd[p + n]
        blocks.append(wb)
    scp, shp = fold_bn(sd, "policy_bn1")
    P, C = sd["policy_conv1.weight"].shape[:2]
    head = {"wp1": sd["policy_conv1.weight"].reshape(P, C), "scp": scp, "shp": shp,
            "wp2": sd["policy_conv2.weight"].reshape(MOVES, P), "bp2": sd["policy_conv2.bias"]}
    for k, n in (("v1", "value_fc1"), ("v2", "value_fc2"), ("s1", "score_fc1"), ("s2", "score_fc2")):
        head[k + "w"], head[k + "b"] = sd[n + ".weight"], sd[n + ".bias"]
    return stem, tuple(blocks), head


# ------------------------------------------------------------------------------------------------ pointer tables


def pack_bytes(Nout: int, Kin: int) -> int:
    """bytes of a bf16 ka_pack_conv3x3 pack: 9 taps x Kin / 32 k-steps x Nout / 16 tiles x 64 fragments of 16 bytes"""
    return 9 * (Kin // 32) * (Nout // 16) * 64 * 16


def table(rows_of_dicts, fields, dev, pack, kin=None):
    """(int64 device table, the tensors it points to -- keep them alive for as long as a launch may read the table).
    rows_of_dicts: nested lists of dicts; every leaf dict becomes a row of len(fields) pointers.  pack(w, Kin) -> device bytes
    for the conv weights (fields w1, w2, w); every other field goes up as a contiguous float32 tensor of its own, which the
    allocator aligns to far more than the 16 bytes the kernels' float4 loads need."""
    keep = []

    def row(d):
        ptrs = []
        for f in fields:
            t = pack(d[f], kin or d[f].shape[1]) if f in ("w1", "w2", "w") else d[f].float().contiguous().to(dev)
            assert t.data_ptr() % 16 == 0
            keep.append(t)
            ptrs.append(t.data_ptr())
        return ptrs

    def walk(n):
        return row(n) if isinstance(n, dict) else [walk(k) for k in n]

    return torch.tensor(walk(list(rows_of_dicts)), dtype=torch.int64).to(dev), keep
