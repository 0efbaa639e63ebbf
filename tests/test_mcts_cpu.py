"""The visit-count search without a GPU: the controls and their table, the refusals, the C ABI, ``visit_policy``, the float64
restatement (``mcts_backup_select``) on hand-made trees, and the condition under which the synthetic worlds of
tests/mcts_helpers.py can be held to it on the device."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mcts_helpers as H
from keisei_amd import _lib, build
from keisei_amd.shogi_gym import ACTION_SPACE
from keisei_amd.training import (LookaheadControls, MctsControls, MctsStats, SearchControls, lookahead_active, lookahead_table,
                                 mcts_backup_select, mcts_simulations, mcts_table, search_records, visit_policy)
from keisei_amd.training.mcts_search import MAX_SIMULATIONS, arena_mcts

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------ controls, table, refusals, ABI
def test_the_controls_are_validated_like_the_tree_searchs():
    c = MctsControls(4, 32, 1.25, 3)
    assert (c.width, c.simulations, c.c_puct, c.skip_plies) == (4, 32, 1.25, 3)
    assert MctsControls(3) == MctsControls(3, 1, 0.0, 0) and MctsControls.OFF == MctsControls()
    for kw, msg in ((dict(width=9), "width must be an integer"), (dict(width=-1), "width must be an integer"),
                    (dict(width=True), "width must be an integer"), (dict(width=2, simulations=0), "simulations must be an integer"),
                    (dict(width=2, simulations=65), "simulations must be an integer"),
                    (dict(width=2, simulations=2.0), "simulations must be an integer"),
                    (dict(width=2, c_puct=-0.1), "c_puct must be finite"),
                    (dict(width=2, c_puct=float("inf")), "c_puct must be finite"),
                    (dict(width=2, c_puct=3.3e38), "fit a float32"),
                    (dict(width=2, skip_plies=65536), "skip_plies must be an integer"),
                    (dict(width=0, simulations=2), "needs a width above 0")):
        with pytest.raises(ValueError, match=msg):
            MctsControls(**kw)


def test_the_table_words_and_how_the_kernel_reads_them():
    t = mcts_table([MctsControls(3, 40, 1.25), MctsControls(2, 1, 0.0, 4)], 2)
    assert t.dtype == np.int32 and t.shape == (2, 4)
    assert t[:, 0].tolist() == [3, 2] and t[:, 2].tolist() == [0, 4] and t[:, 3].tolist() == [40, 1]
    assert t[:, 1].view(np.float32).tolist() == [1.25, 0.0]
    # words 0-2 are the lookahead's, and an env is active by its rule
    la = lookahead_table([LookaheadControls(3, 1.25), LookaheadControls(2, 0.0, 4)], 2)
    assert np.array_equal(t[:, :3], la[:, :3])
    widths, _ = lookahead_active(t, [0, 1, 1, -1, 2], [0, 3, 4, 0, 0])
    assert widths.tolist() == [3, 0, 2, 0, 0]
    assert mcts_table(None, 3)[:, 3].tolist() == [1, 1, 1] and not mcts_table(None, 3)[:, :3].any()
    # word 3 outside [1, 64] reads as 1, a model outside [0, K) too; the launch's simulations cut it
    raw = t.copy()
    raw[0, 3] = 65
    raw[1, 3] = 0
    assert mcts_simulations(raw, [0, 1, -1, 2])[1].tolist() == [1, 1, 1, 1]
    assert mcts_simulations(t, [0, 1], simulations=8)[1].tolist() == [8, 1]
    assert mcts_simulations(t, [0, 1])[0].tolist() == [1.25, 0.0]
    for bad, msg in ((([MctsControls(1)] * 2, 3), "expected 3"), (([SearchControls(1)], 1), "must be a MctsControls"),
                     ((MctsControls(1), 0), "at least one row"), (("x", 1), "mcts must be None")):
        with pytest.raises(ValueError, match=msg):
            mcts_table(*bad)


def test_the_arenas_reading_and_its_refusals():
    assert arena_mcts(None, 2, False) == (None, 0, 0) and arena_mcts(None, 2, True, LookaheadControls(2)) == (None, 0, 0)
    table, width, sims = arena_mcts([MctsControls(3, 40, 1.25), MctsControls(2, 1, 0.0, 4)], 2, False)
    assert (width, sims) == (3, 40) and table.shape == (2, 4)
    assert arena_mcts(MctsControls.OFF, 2, False)[1:] == (0, 1)
    with pytest.raises(ValueError, match="cannot be combined with lookahead="):
        arena_mcts(MctsControls(2, 2), 2, False, LookaheadControls(2))
    with pytest.raises(ValueError, match="cannot be combined with search="):
        arena_mcts(MctsControls(2, 2), 2, False, None, SearchControls(2, 2))
    with pytest.raises(ValueError, match="cannot be combined with collect=True"):
        arena_mcts(MctsControls(2, 2), 2, True)
    assert MctsStats() == MctsStats(0, 0, 0, 0, 0, 0)


def test_the_symbols_are_exported_declared_bound_and_built():
    names = ("ka_mcts_words", "ka_mcts_advance")
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    lib = ctypes.CDLL(str(_lib.library_path()))
    for n in names:
        assert re.search(rf"\bint {n}\(", header) and hasattr(lib, n) and n in _lib._SIGS and n in _lib.exported_symbols(), n
    assert "mcts.hip" in build.SOURCES
    assert len(_lib._SIGS["ka_mcts_words"].replace(" ", "")) == 3
    assert len(_lib._SIGS["ka_mcts_advance"].replace(" ", "")) == 23
    q = lambda *a: _lib.query("ka_mcts_words", *a)  # noqa: E731
    assert q(0, 3, 4) == 4 + 9 and q(1, 3, 4) == 4 + 4 * 12 and q(1, 8, 64) == 64 + 4 * 512 and q(2, 1, 1) == 6
    assert q(3, 0, 0) == 8 and q(4, 0, 0) == 64 == MAX_SIMULATIONS and q(5, 0, 0) == 4
    assert q(0, 9, 1) == -1 and q(0, 1, 65) == -1 and q(6, 1, 1) == -1


def test_visit_policy_sums_to_one_on_the_candidates_and_is_one_hot_at_zero():
    cand = torch.tensor([[7, 11258, 40, -1], [5, 6, -1, -1], [-1, -1, -1, -1], [9, 8, 7, 6]])
    vis = torch.tensor([[3, 1, 4, 0], [2, 2, 0, 0], [0, 0, 0, 0], [1, 5, 5, 1]], dtype=torch.int32)
    p = visit_policy(cand, vis)
    assert p.dtype == torch.float32 and p.shape == (4, ACTION_SPACE)
    assert torch.allclose(p.sum(1), torch.tensor([1.0, 1.0, 0.0, 1.0]), atol=1e-6)
    assert p[0, [7, 11258, 40]].tolist() == pytest.approx([3 / 8, 1 / 8, 4 / 8]) and p[1, [5, 6]].tolist() == [0.5, 0.5]
    for row in range(4):                                      # nothing outside the candidates
        rest = torch.ones(ACTION_SPACE, dtype=torch.bool)
        rest[cand[row][cand[row] >= 0]] = False
        assert not p[row][rest].any()
    sharp = visit_policy(cand, vis, temperature=0.5)          # visits ** 2
    assert sharp[0, [7, 11258, 40]].tolist() == pytest.approx([9 / 26, 1 / 26, 16 / 26])
    hot = visit_policy(cand, vis, temperature=0)
    assert hot.sum(1).tolist() == [1.0, 1.0, 0.0, 1.0]
    assert hot[0, 40] == 1 and hot[1, 5] == 1 and hot[3, 8] == 1          # ties keep the lower slot: the choice
    for bad, msg in (((cand, vis, -1.0), "temperature"), ((cand, vis[:, :3]), "both"), ((cand, vis + 1), "names no action")):
        with pytest.raises(ValueError, match=msg):
            visit_policy(*bad)


# ------------------------------------------------------------------ the restatement on hand-made trees
def _drive(worlds, W, E, controls, model_of=None):
    """Search hand-made trees: ``worlds[b]`` is a dict from the slots behind a node (a tuple, () = the root) to its children,
    a list of ``(q, prior, done)`` of at most W; a path that is not in it has no candidates.  Every simulation goes where
    the restatement sent it; returns the tree after each simulation and the ``parent`` array."""
    B = len(worlds)
    n_cand, q, pri = np.zeros((E, B), np.int64), np.zeros((E, B, W)), np.zeros((E, B, W))
    done, parent = np.zeros((E, B, W), bool), np.full((E, B), -1, np.int64)
    paths = [{} for _ in range(B)]
    trees = []
    for t in range(E):
        for b in range(B):
            node = -1 if t == 0 else int(trees[-1].next_node[b])
            if t > 0 and node < 0:
                continue
            parent[t, b] = node
            path = () if t == 0 else paths[b][node]
            kids = worlds[b].get(path, []) if t == 0 or trees[-1].fork_next[b] else []
            assert len(kids) <= W
            n_cand[t, b] = len(kids)
            for j, (v, p, d) in enumerate(kids):
                q[t, b, j], pri[t, b, j], done[t, b, j], paths[b][t * W + j] = v, p, d, path + (j,)
        rec = search_records(n_cand[:t + 1], pri[:t + 1], q[:t + 1])
        trees.append(mcts_backup_select(rec, done[:t + 1], parent[:t + 1], controls, model_of, q=q[:t + 1]))
    return trees, parent


HAND = {(): [(0.25, 0.75, False), (0.5, 0.25, False)],                # A, B
        (0,): [(0.125, 0.5, False), (0.625, 0.5, False)],             # behind A
        (1,): [(-0.5, 1.0, False), (-0.25, 0.0, False)],              # behind B
        (1, 0): [(0.375, 0.5, False), (0.125, 0.5, False)]}           # behind B's first child


def test_a_hand_worked_tree_of_width_2_and_4_simulations():
    """c_puct = 1, every q on the 1/8 grid.  Worked by hand:
    simulation 1: Npar 2; A 0.25 + 0.75 sqrt(2) / 2, B 0.5 + 0.25 sqrt(2) / 2 -> A, a leaf; its children's best q is 0.625, so
      A: N 2, S 0.25 - 0.625 = -0.375.
    simulation 2: Npar 3; A -0.1875 + 0.75 sqrt(3) / 3, B 0.5 + 0.25 sqrt(3) / 2 -> B, a leaf; best q behind it -0.25, so
      B: N 2, S 0.5 + 0.25 = 0.75.
    simulation 3: Npar 4; A -0.1875 + 0.75 * 2 / 3 = 0.3125, B 0.375 + 0.25 * 2 / 3 -> B; behind it Npar 2; first child
      -0.5 + sqrt(2) / 2, second -0.25 + 0 -> the first, a leaf; best q behind it 0.375, so it gets N 2, S -0.875 and B
      N 3, S 0.75 + 0.375 = 1.125.
    B has 3 visits of 5: the choice, the one-ply choice as well."""
    r2, r3 = math.sqrt(2), math.sqrt(3)
    trees, parent = _drive([HAND], 2, 4, MctsControls(2, 4, 1.0))
    assert parent[:, 0].tolist() == [-1, 0, 1, 4]
    want_scores = {1: [(0, [0.25 + 0.75 * r2 / 2, 0.5 + 0.25 * r2 / 2], 0)],
                   2: [(0, [-0.1875 + 0.75 * r3 / 3, 0.5 + 0.25 * r3 / 2], 1)],
                   3: [(0, [0.3125, 0.375 + 0.25 * 2 / 3], 1), (2, [-0.5 + r2 / 2, -0.25], 0)]}
    sel = trees[-1].selections
    assert sel[3][0] == []                                    # the last simulation selects nothing
    for t, levels in want_scores.items():
        got = sel[t - 1][0]                                   # made behind simulation t - 1
        assert [(x, k) for x, _, k in got] == [(x, k) for x, _, k in levels], t
        for (_, g, _), (_, w, _) in zip(got, levels):
            assert g.tolist() == pytest.approx(w, abs=1e-15), t
    assert [tr.next_node[0] for tr in trees] == [0, 1, 4, -1] and [bool(tr.fork_next[0]) for tr in trees] == [True, True, True, False]
    N = [[[1, 1]], [[2, 1], [1, 1]], [[2, 2], [1, 1], [1, 1]], [[2, 3], [1, 1], [2, 1], [1, 1]]]
    S = [[[0.25, 0.5]], [[-0.375, 0.5], [0.125, 0.625]], [[-0.375, 0.75], [0.125, 0.625], [-0.5, -0.25]],
         [[-0.375, 1.125], [0.125, 0.625], [-0.875, -0.25], [0.375, 0.125]]]
    for t, tr in enumerate(trees):
        assert tr.N[0].tolist() == N[t] and tr.S[0].tolist() == S[t] and tr.S32[0].tolist() == S[t], t     # exact on the grid
        assert not tr.revisit.any() and tr.ran[:, 0].all()
    last = trees[-1]
    assert last.by[0].tolist() == [[1, 2], [-1, -1], [3, -1], [-1, -1]]
    assert last.P[0].tolist() == [[0.75, 0.25], [0.5, 0.5], [1.0, 0.0], [0.5, 0.5]]
    assert last.choice[0] == 1 and last.one_ply[0] == 1 and not last.deepened[0]
    assert last.visits[0].tolist() == [2, 3] and last.mean[0].tolist() == [-0.1875, 0.375]
    assert last.slot[:, 0].tolist() == [1, -1, 0, -1]         # the slots last selected among each simulation's children
    assert last.pv[0].tolist() == [1, 2 * 2 + 0, 3 * 2 + 0, -1]           # B, its more visited child, a tie behind it
    assert trees[1].choice[0] == 0 and trees[1].deepened[0]   # after two simulations A has the visits, B the better q


def test_a_model_with_fewer_simulations_stops_selecting_and_chooses_there():
    ctl = [MctsControls(2, 4, 1.0), MctsControls(2, 2, 1.0)]
    trees, parent = _drive([HAND, HAND], 2, 4, ctl, model_of=[0, 1])
    assert parent[:, 0].tolist() == [-1, 0, 1, 4] and parent[:, 1].tolist() == [-1, 0, -1, -1]
    assert trees[1].next_node.tolist() == [1, -1] and trees[-1].ran[:, 1].tolist() == [True, True, False, False]
    two = trees[1]                                            # what both rows were after two simulations
    for tr in trees[1:]:
        assert tr.N[1, :2].tolist() == two.N[0].tolist() and tr.choice[1] == two.choice[0] == 0 and tr.deepened[1]
        assert tr.visits[1].tolist() == [2, 1] and tr.pv[1, :2].tolist() == [0, 2] and (tr.pv[1, 2:] == -1).all()
    assert trees[-1].choice.tolist() == [1, 0] and not trees[-1].N[1, 2:].any()
    assert mcts_simulations(ctl, [0, 1], simulations=3)[1].tolist() == [3, 2]


def test_a_done_child_that_keeps_winning_is_revisited_and_counted():
    world = {(): [(1.0, 0.5, True), (0.5, 0.5, False)]}       # a winning move that ends the game, and another
    trees, parent = _drive([world], 2, 4, MctsControls(2, 4, 0.0))
    assert parent[:, 0].tolist() == [-1, 0, 0, 0] and [bool(tr.fork_next[0]) for tr in trees] == [False] * 4
    last = trees[-1]
    assert last.revisit[:, 0].tolist() == [False, True, True, True] and last.ran[:, 0].all()
    assert last.N[0, 0].tolist() == [4, 1] and last.S[0, 0].tolist() == [4.0, 0.5] and (last.by[0] == -1).all()
    assert last.choice[0] == 0 and last.pv[0].tolist() == [0, -1, -1, -1] and last.mean[0].tolist() == [1.0, 0.5]
    # a node forked without a candidate is revisited in the same way, with its own q; the signs alternate above it
    world = {(): [(0.5, 0.5, False)], (0,): [(-0.25, 0.5, False)]}
    trees, parent = _drive([world], 1, 4, MctsControls(1, 4, 0.0))
    last = trees[-1]
    assert parent[:, 0].tolist() == [-1, 0, 1, 1] and last.revisit[:, 0].tolist() == [False, False, True, True]
    assert last.N[0, :2, 0].tolist() == [4, 3] and last.S[0, :2, 0].tolist() == [0.5 + 0.25 + 0.25 + 0.25, -0.25 * 3]


def test_c_puct_zero_is_greedy_on_the_mean_value():
    world = H.make_world(3, 5, 5, n_rows=16)
    world["ctl"] = [MctsControls(3, 5, 0.0)] * 2
    r, _ = H.walk_restatement(world)
    seen = 0
    for sel in r.selections:
        for b, levels in enumerate(sel):
            for x, scores, k in levels:
                # (the tree moved on since; the scores themselves are means: no prior term, and the first maximum is taken)
                assert k == int(np.argmax(scores)) and np.all(np.abs(scores) <= 1.0)
                seen += 1
    assert seen > 50
    # and on the hand-worked tree: B's mean stays above A's, so every simulation goes down B, and behind B to the child
    # with the better q, which has no move: it is revisited
    trees, parent = _drive([HAND], 2, 4, MctsControls(2, 4, 0.0))
    assert parent[:, 0].tolist() == [-1, 1, 3, 3] and trees[-1].revisit[:, 0].tolist() == [False, False, True, True]
    (x0, s0, k0), (x1, s1, k1) = trees[-1].selections[2][0]   # the selection of simulation 3
    assert (x0, k0, x1, k1) == (0, 1, 1, 1) and s0.tolist() == [0.25, 1.0 / 3] and s1.tolist() == [-0.5, -0.25]
    assert trees[-1].N[0, :2].tolist() == [[1, 4], [1, 3]] and trees[-1].S[0, :2].tolist() == [[0.25, 1.25], [-0.5, -0.75]]


def test_one_simulation_plays_slot_0():
    world = H.make_world(4, 1, 9, n_rows=16)
    r, bad = H.walk_restatement(world)
    tr = r.tree()
    root = world["n_all"][0] > 0
    assert tr.choice.tolist() == np.where(root, 0, -1).tolist() and not bad and not tr.selections[0][1]
    assert np.array_equal(tr.pv[:, 0], np.where(root, world["cands"][0, :, 0], -1))
    assert tr.visits[root].max() == 1 and (tr.next_node == -1).all()


def test_the_restatement_in_one_call_is_the_restatement_step_by_step():
    world = H.make_world(3, 5, 6, n_rows=16)
    r, _ = H.walk_restatement(world)
    step = r.tree()
    W = 3
    rec = np.stack([H.record_of(world, t, r.ran[t] & ~r.revisit[t] if t else np.ones(16, bool)) for t in range(5)])
    rec.view(np.float32)[:, :, 4 + 2 * W:] = r.q.transpose(1, 0, 2).astype(np.float32)
    once = mcts_backup_select(rec, world["done"], r.parent, world["ctl"], world["model_of"])
    for name in ("N", "S", "by", "ran", "revisit", "choice", "pv", "visits", "mean", "deepened"):
        assert np.array_equal(getattr(once, name), getattr(step, name)), name


# ------------------------------------------------------------------ the generator condition
@pytest.mark.parametrize("W,E", H.SHAPES)
def test_no_selection_of_the_synthetic_worlds_is_closer_than_fp32_can_tell(W, E):
    """What tests/test_hip_mcts.py relies on: walked with the restatement as the chooser, every selection of the world of
    ``H.SEEDS[W, E]`` has its two best scores either computed from bit-identical (S, N, P) or at least 1e-3 apart, at every
    node -- none is left out.  ``make_world`` draws a row again until it is so (rows do not see each other; about one row in
    five of the (8, 64) world needs it): PUCT brings the best scores of a node together by design, and no seed of 64 rows by
    64 simulations is free of close calls otherwise."""
    world = H.make_world(W, E, H.SEEDS[W, E])
    r, bad = H.walk_restatement(world)
    assert bad == []
    levels = sum(len(s) for sel in r.selections for s in sel)
    tr = r.tree()
    root = tr.choice >= 0
    assert root.sum() == H.B - 1 and not root[0] and world["n_all"][0, 1] == 1
    assert len(set(world["model_of"].tolist())) == 2
    if E > 1:                                                 # and the walk is worth holding a kernel to
        chosen = world["cands"][0][np.arange(H.B), np.maximum(tr.choice, 0)]
        changed = root & (chosen != world["sampled"])
        assert levels > H.B * (E - 1) // 2 and tr.revisit.sum() >= 1 and tr.deepened.sum() >= 1
        assert changed.sum() >= 1 and (root & ~changed).sum() >= 1
        contested = sum(1 for sel in r.selections for s in sel for _, scores, _ in s if len(scores) > 1)
        assert contested > levels // 2


def test_the_shared_table_reader_and_field_checks():
    from test_lookahead_cpu import check_field_refusals, check_table_of
    check_table_of(mcts_table, "mcts", MctsControls(3, 4, 1.25), [MctsControls(3, 4, 1.25, 2), MctsControls()])
    check_field_refusals(lambda **kw: MctsControls(**dict({"width": 1}, **kw)),
                         ints=(("width", 8), ("skip_plies", 65535), ("simulations", MAX_SIMULATIONS)), weights=("c_puct",))
