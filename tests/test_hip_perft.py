"""csrc/perft.hip behind VecEnv.perft / perft_divide against the C oracle: the known counts of tests/perft_helpers.py and
their mirrors, chunked walks at the smallest shapes, every column against the oracle env's walk, games that end inside the
tree, the divide per action, the fork and the plan alone, and an env that is only read."""
import numpy as np
import pytest
import torch

import perft_helpers as P
from keisei_amd import _lib
from keisei_amd.perft import MAX_MOVES, perft_plan_host
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS, VecEnv, parse_sfen
from oracle import shogi as S
from oracle.shogi import OracleVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _env(sfens, max_ply=500):
    env = VecEnv(len(sfens), max_ply, "katago", "spatial")
    env.reset()
    pos = [parse_sfen(s) for s in sfens]
    env.set_states(np.stack([p[0] for p in pos]), np.stack([p[1] for p in pos]), np.array([p[2] for p in pos], np.uint8))
    return env


def _batch(min_depth):
    """(names, sfens, counts) of the table rows that list at least ``min_depth`` depths, each followed by its mirror."""
    names = [n for n in P.NAMES if len(P.TABLE[n][1]) >= min_depth]
    sfens = [s for n in names for s in (P.TABLE[n][0], P.MIRRORS[n])]
    return [n for n in names for _ in range(2)], sfens, [P.TABLE[n][1] for n in names for _ in range(2)]


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_the_table_and_its_mirrors_in_one_batch(depth):
    """All rows (and mirrors) that list this depth in one env batch; every shallower depth is read from by_depth."""
    names, sfens, counts = _batch(depth)
    assert len(names) == {2: 14, 3: 12, 4: 2}[depth]
    res = _env(sfens).perft(depth, rows=32768)
    assert res.nodes.dtype == res.by_depth.dtype == np.uint64 and res.by_depth.shape == (len(sfens), depth, 4)
    for e, (name, want) in enumerate(zip(names, counts)):
        assert res.by_depth[e, :, 0].tolist() == list(want[:depth]), (name, e)
        assert int(res.nodes[e]) == want[depth - 1], (name, e)
    assert (res.by_depth[:, :, 2] == 0).all()                            # no game ended other than by mate
    assert (res.by_depth[:, depth - 1, 1:] == 0).all()                   # bulk: the last depth carries nodes only
    if depth == 2:                                                       # depth 1 comes from the masks alone
        one = _env(sfens).perft(1)
        assert one.nodes.tolist() == [c[0] for c in counts] and one.chunks == 0


@pytest.mark.parametrize("name, rows", [("evasion", 8), ("start", 64)])
def test_a_small_rows_splits_the_walk_and_counts_the_same(name, rows):
    sfen, want = P.TABLE[name]
    env = _env([sfen, P.MIRRORS[name]])
    res = env.perft(3, rows=rows)
    assert res.by_depth[:, :, 0].tolist() == [list(want[:3])] * 2 and res.nodes.tolist() == [want[2]] * 2
    assert res.chunks > 2                                                # two levels are forked: more launches than levels
    level2 = 2 * want[1]
    assert res.chunks >= 1 + -(-level2 // rows)                          # the second level alone cannot fit fewer chunks
    whole = env.perft(3, rows=32768)
    assert whole.chunks == 2 and (whole.by_depth == res.by_depth).all()
    full = env.perft(3, rows=MAX_MOVES, bulk=False)                      # (the third level is forked too: room for any position)
    assert full.nodes.tolist() == res.nodes.tolist() and full.chunks >= 3


def test_rows_smaller_than_a_positions_moves_raise():
    env = _env([P.START])
    with pytest.raises(ValueError, match=r"row 0 of level 0 has 30 legal moves.*593"):
        env.perft(2, rows=16)
    big = _env([P.TABLE["max593"][0]])
    assert big.perft(2, rows=MAX_MOVES).nodes.tolist() == [P.TABLE["max593"][1][1]]
    with pytest.raises(ValueError, match=r"has 593 legal moves.*rows=592"):
        big.perft(2, rows=MAX_MOVES - 1)
    for bad in (dict(depth=0), dict(depth=9), dict(depth=2, rows=0), dict(depth=True)):
        with pytest.raises(ValueError):
            env.perft(**bad)
    with pytest.raises(ValueError, match="katago"):
        VecEnv(1, 100, "default", "default").perft(1)


def test_every_column_equals_the_oracle_envs_walk():
    names = ("evasion", "pawn_drop", "gold_head")
    sfens = [P.TABLE["evasion"][0], P.TABLE["pawn_drop"][0], P.GOLD_HEAD]
    sfens = sfens + [P.mirror_sfen(s) for s in sfens]
    env = _env(sfens)
    full, bulk = env.perft(3, bulk=False), env.perft(3)
    assert full.nodes.tolist() == bulk.nodes.tolist()
    assert (full.by_depth[:, :2] == bulk.by_depth[:, :2]).all()
    for e, s in enumerate(sfens):
        want = P.env_perft(s, 3)
        assert (full.by_depth[e] == want).all(), (names[e % 3], e, full.by_depth[e].tolist(), want.tolist())
    gold = names.index("gold_head")
    assert full.by_depth[gold, :, 1].sum() > 0 and full.by_depth[gold + 3, :, 1].sum() > 0      # mates inside the tree
    assert full.by_depth[:, :, 3].sum() > 0


def test_games_that_end_by_the_move_limit_have_no_successors():
    env = _env([P.START], max_ply=2)
    want = P.env_perft(P.START, 3, 2)
    full = env.perft(2, bulk=False)
    assert full.by_depth[0, :, 0].tolist() == [30, 900]
    assert full.by_depth[0, :, 2].tolist() == [0, 900] and full.by_depth[0, :, 1].sum() == 0
    assert (full.by_depth[0] == want[:2]).all()
    three = env.perft(3)
    assert three.nodes.tolist() == [0] and three.by_depth[0, :, 0].tolist() == [30, 900, 0]
    assert three.by_depth[0, 1, 2] == 900
    assert (env.perft(3, bulk=False).by_depth[0] == want).all()


@pytest.mark.parametrize("name", ["start", "mid_drops"])
def test_divide_equals_the_oracle_per_action(name):
    sfen, want = P.TABLE[name]
    board, hands, side = parse_sfen(sfen)
    env = _env([sfen, P.START])
    got = env.perft_divide(3)
    assert len(got) == 2 and sum(got[0].values()) == want[2] and sum(got[1].values()) == P.TABLE["start"][1][2]
    assert list(got[0]) == sorted(got[0]) and len(got[0]) == want[0]
    ref = OracleVecEnv(1, 500)
    ref.reset()
    for a, leaves in got[0].items():
        frm, to, promote, drop = S.decode(a, white=bool(side))
        ref.set_state(0, board, hands, side)
        ref.play(0, frm, to, bool(promote), drop)
        assert ref.perft(2) == leaves, (name, a)
    assert int(env.perft(3).nodes[0]) == want[2]
    one = env.perft_divide(1)
    assert one[0] == {a: 1 for a in got[0]} and env.perft_divide(2)[1] == {a: 30 for a in got[1]}


def _fork_rows(hist, ply, cap):
    g = torch.Generator().manual_seed(3)
    state = torch.randint(0, 256, (1, 128), dtype=torch.uint8, generator=g)
    state[0, 100:104] = torch.tensor([ply, 0, 0, 0], dtype=torch.uint8)
    keys = torch.randint(1, 1 << 60, (1, hist), dtype=torch.int64, generator=g)
    checks = torch.randint(0, 2, (1, hist), dtype=torch.uint8, generator=g)
    bits = np.zeros(MASK_WORDS, np.uint32)
    for a in (0, 31, 32, ACTION_SPACE - 1):
        bits[a >> 5] |= np.uint32(1) << np.uint32(a & 31)
    bits[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(ACTION_SPACE & 31)    # every bit past the action space
    mask = torch.from_numpy(bits.view(np.int32).copy())[None]
    parent = [t.to(DEV) for t in (state, mask, keys, checks)]
    def fill(*shape, dtype):                                             # every byte 0x55
        size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return torch.full((size,), 0x55, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)

    child = dict(state=fill(cap, 128, dtype=torch.uint8), keys=fill(cap, hist, dtype=torch.int64),
                 checks=fill(cap, hist, dtype=torch.uint8), bits=fill(cap, MASK_WORDS, dtype=torch.int32),
                 actions=fill(cap, dtype=torch.int64), tag=fill(cap, dtype=torch.int32))
    return parent, child


def _fork(parent, child, moves, offset, tag, cap, base, max_ply):
    state, mask, keys, checks = parent
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)  # noqa: E731
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.call("ka_perft_fork", state, mask, MASK_WORDS, keys, checks, i32(moves), i32(offset), i32(tag), 0, 1, 1, max_ply, cap,
              base, child["state"], child["keys"], child["checks"], child["bits"], child["actions"], child["tag"], err,
              ACTION_SPACE, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return int(err.item())


@pytest.mark.parametrize("hist, base", [(16, -1), (7, 100)])
def test_the_fork_alone_on_a_hand_made_parent(hist, base):
    ply, cap, off = 3, 8, 2
    parent, child = _fork_rows(hist, ply, cap)
    assert _fork(parent, child, 4, off, 7, cap, base, hist) == 0
    rows = slice(off, off + 4)
    assert child["actions"][rows].tolist() == [0, 31, 32, ACTION_SPACE - 1]          # ascending, the tail bits dropped
    assert child["tag"][rows].tolist() == ([7] * 4 if base < 0 else [base + off + r for r in range(4)])
    state, mask, keys, checks = parent
    assert (child["state"][rows] == state).all() and (child["bits"][rows] == mask).all()
    assert (child["keys"][rows, :ply] == keys[:, :ply]).all() and (child["checks"][rows, :ply] == checks[:, :ply]).all()
    for name, t in child.items():                                        # no row outside offset + [0, moves) is touched
        rest = torch.cat([t[:off], t[off + 4:]]).cpu().numpy()
        assert (rest.view(np.uint8) == 0x55).all(), name


def test_the_fork_refuses_what_would_leave_its_rows():
    parent, child = _fork_rows(16, 3, 8)
    untouched = lambda: all((t.cpu().numpy().view(np.uint8) == 0x55).all() for t in child.values())  # noqa: E731
    assert _fork(parent, child, 4, 5, 7, 8, -1, 16) == 1 and untouched()         # rows 5..8 of 8
    assert _fork(parent, child, 0, 0, 7, 8, -1, 16) == 0 and untouched()         # an ended parent forks nothing
    assert _fork(parent, child, 3, 0, 7, 8, -1, 16) == 2                         # the mask has four moves, not three
    assert (child["actions"][3:].cpu().numpy().view(np.uint8) == 0x55).all() and child["actions"][:3].tolist() == [0, 31, 32]
    state, mask, keys, checks = parent
    with pytest.raises(_lib.KeiseiHipError, match="overlap"):
        _fork(parent, dict(child, state=state), 4, 0, 7, 1, -1, 16)
    with pytest.raises(_lib.KeiseiHipError, match="overlap"):
        _fork(parent, dict(child, bits=mask), 4, 0, 7, 1, -1, 16)


def _plan(moves, cursor, cap):
    n = len(moves)
    m = torch.tensor(moves, dtype=torch.int32, device=DEV)
    offset = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    header = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    _lib.call("ka_perft_plan", m, cursor, n, cap, offset, header, _lib.stream_ptr(torch.device(DEV)))
    return header.tolist(), offset.tolist()


@pytest.mark.parametrize("moves, cursor, cap, want", P.PLAN_CASES)
def test_the_plan_kernel_on_the_edge_lists(moves, cursor, cap, want):
    header, offset = _plan(moves, cursor, cap)
    taken, children, blocking, offsets = perft_plan_host(moves, cursor, cap)
    assert tuple(header) == want == (taken, children, blocking)
    assert offset[cursor:cursor + taken] == offsets
    assert all(v == -7 for v in offset[:cursor] + offset[cursor + taken:])       # nothing else is written


@pytest.mark.parametrize("cap", [MAX_MOVES, 2048, 1 << 20])
def test_the_plan_kernel_on_random_counts(cap):
    moves = np.random.default_rng(11).integers(0, MAX_MOVES + 1, 4096).tolist()
    m = torch.tensor(moves, dtype=torch.int32, device=DEV)
    offset = torch.zeros(4096, dtype=torch.int32, device=DEV)
    header = torch.zeros(3, dtype=torch.int32, device=DEV)
    cursor, chunks = 0, 0
    while cursor < 4096:                                                 # the walk of one level, chunk by chunk
        _lib.call("ka_perft_plan", m, cursor, 4096, cap, offset, header, _lib.stream_ptr(torch.device(DEV)))
        taken, children, blocking, offsets = perft_plan_host(moves, cursor, cap)
        assert header.tolist() == [taken, children, blocking] and taken > 0
        assert offset[cursor:cursor + taken].tolist() == offsets
        cursor, chunks = cursor + taken, chunks + 1
    assert 2 ** 20 < sum(moves) < 2 ** 21                                # (the largest cap: one full chunk and the rest)
    assert chunks == 2 if cap == 1 << 20 else chunks > 4096 * 250 // cap


def _played(seed, plies):
    """An env of 4 games after ``plies`` seeded random legal moves (numpy output), and the actions played."""
    env = VecEnv(4, 200, "katago", "spatial")
    mask = env.reset().legal_masks
    rng = np.random.default_rng(seed)
    for _ in range(plies):
        mask = env.step([int(rng.choice(np.flatnonzero(m))) for m in mask]).legal_masks
    return env, rng


def test_the_env_is_only_read():
    env, rng = _played(9, 5)
    twin, _ = _played(9, 5)
    snap = lambda e: [t.clone() for t in (e._state, e._keys, e._checks, *e._bits, *e._mask, *e._obs, e._stats, e._err)]  # noqa: E731
    before = snap(env)
    assert all(torch.equal(a, b) for a, b in zip(before, snap(twin)))
    res = env.perft(3, rows=1024)
    assert res.chunks > 2 and (res.by_depth[:, 0, 0] > 0).all() and (res.nodes > res.by_depth[:, 1, 0]).all()
    assert sum(env.perft_divide(2)[0].values()) == int(res.by_depth[0, 1, 0])
    assert all(torch.equal(a, b) for a, b in zip(before, snap(env)))
    mask = env.current().legal_masks
    assert (mask == twin.current().legal_masks).all()
    for _ in range(12):
        acts = [int(rng.choice(np.flatnonzero(m))) for m in mask]
        a, b = env.step(acts), twin.step(acts)
        for f in ("observations", "legal_masks", "rewards", "terminated", "truncated", "current_players"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        mask = a.legal_masks
    assert all(torch.equal(x, y) for x, y in zip(snap(env), snap(twin)))
