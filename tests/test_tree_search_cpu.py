"""The tree search without a GPU: the controls and their table, the refusals, the C ABI, and the float64 restatement
(``search_backup_select``) on hand-made trees, one tree per case."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training import (LookaheadControls, SearchControls, SearchStats, lookahead_active, lookahead_choose,
                                 lookahead_table, search_backup_select, search_expansions, search_leaf_q, search_records,
                                 search_table)
from keisei_amd.training.tree_search import ERR_VALUE, MAX_EXPANSIONS, arena_search

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------ controls, table, refusals, ABI
def test_the_controls_are_validated_like_the_lookaheads():
    c = SearchControls(4, 8, 0.25, 3)
    assert (c.width, c.expansions, c.prior_weight, c.skip_plies) == (4, 8, 0.25, 3)
    assert SearchControls(3) == SearchControls(3, 1, 0.0, 0) and SearchControls.OFF == SearchControls()
    for kw, msg in ((dict(width=9), "width must be an integer"), (dict(width=-1), "width must be an integer"),
                    (dict(width=True), "width must be an integer"), (dict(width=2, expansions=0), "expansions must be an integer"),
                    (dict(width=2, expansions=17), "expansions must be an integer"),
                    (dict(width=2, expansions=2.0), "expansions must be an integer"),
                    (dict(width=2, prior_weight=-0.1), "prior_weight must be finite"),
                    (dict(width=2, prior_weight=float("nan")), "prior_weight must be finite"),
                    (dict(width=2, prior_weight=3.3e38), "fit a float32"),
                    (dict(width=2, skip_plies=65536), "skip_plies must be an integer"),
                    (dict(width=0, expansions=2), "needs a width above 0")):
        with pytest.raises(ValueError, match=msg):
            SearchControls(**kw)


def test_the_table_words_and_how_the_kernels_read_them():
    t = search_table([SearchControls(3, 4, 0.25), SearchControls(2, 1, 0.0, 4)], 2)
    assert t.dtype == np.int32 and t.shape == (2, 4)
    assert t[:, 0].tolist() == [3, 2] and t[:, 2].tolist() == [0, 4] and t[:, 3].tolist() == [4, 1]
    assert t[:, 1].view(np.float32).tolist() == [0.25, 0.0]
    # words 0-2 are the lookahead's: its table with the same values differs in word 3 alone, and its reader takes this one
    la = lookahead_table([LookaheadControls(3, 0.25), LookaheadControls(2, 0.0, 4)], 2)
    assert np.array_equal(t[:, :3], la[:, :3])
    widths, weights = lookahead_active(t, [0, 1, 1, -1, 2], [0, 3, 4, 0, 0])
    assert widths.tolist() == [3, 0, 2, 0, 0] and weights.tolist()[:3] == [0.25, 0.0, 0.0]
    assert search_table(None, 3)[:, 3].tolist() == [1, 1, 1] and not search_table(None, 3)[:, :3].any()
    assert search_table(SearchControls(2, 5), 2)[:, 3].tolist() == [5, 5]
    # word 3 outside [1, 16] reads as 1, a model outside [0, K) too; the launch's expansions cut it
    raw = t.copy()
    raw[0, 3] = 17
    raw[1, 3] = 0
    assert search_expansions(raw, [0, 1, -1, 2])[1].tolist() == [1, 1, 1, 1]
    assert search_expansions(t, [0, 1], expansions=2)[1].tolist() == [2, 1]
    assert search_expansions(t, [0, 1])[0].tolist() == [0.25, 0.0]
    for bad, msg in ((([SearchControls(1)] * 2, 3), "expected 3"), (([LookaheadControls(1)], 1), "must be a SearchControls"),
                     ((SearchControls(1), 0), "at least one row"), (("x", 1), "search must be None")):
        with pytest.raises(ValueError, match=msg):
            search_table(*bad)


def test_the_arenas_reading_and_its_refusals():
    assert arena_search(None, 2, False) == (None, 0, 0) and arena_search(None, 2, True, LookaheadControls(2)) == (None, 0, 0)
    table, width, expansions = arena_search([SearchControls(3, 4, 0.25), SearchControls(2, 1, 0.0, 4)], 2, False)
    assert (width, expansions) == (3, 4) and table.shape == (2, 4)
    assert arena_search(SearchControls.OFF, 2, False)[1:] == (0, 1)
    with pytest.raises(ValueError, match="cannot be combined with lookahead="):
        arena_search(SearchControls(2, 2), 2, False, LookaheadControls(2))
    with pytest.raises(ValueError, match="cannot be combined with collect=True"):
        arena_search(SearchControls(2, 2), 2, True)
    assert SearchStats() == SearchStats(0, 0, 0, 0, 0)


def test_the_symbols_are_exported_declared_and_bound():
    names = ("ka_search_words", "ka_search_expand", "ka_search_advance")
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    lib = ctypes.CDLL(str(_lib.library_path()))
    for n in names:
        assert re.search(rf"\bint {n}\(", header) and hasattr(lib, n) and n in _lib._SIGS and n in _lib.exported_symbols(), n
    assert len(_lib._SIGS["ka_search_words"].replace(" ", "")) == 3
    assert len(_lib._SIGS["ka_search_expand"].replace(" ", "")) == 27
    assert len(_lib._SIGS["ka_search_advance"].replace(" ", "")) == 21
    q = lambda *a: _lib.query("ka_search_words", *a)  # noqa: E731
    assert q(0, 3, 4) == 4 + 9 and q(1, 3, 4) == 4 + 2 * 12 and q(1, 8, 16) == 16 + 256 and q(2, 1, 1) == 5
    assert q(3, 0, 0) == 8 and q(4, 0, 0) == 16 == MAX_EXPANSIONS and q(5, 0, 0) == 4
    assert q(0, 9, 1) == -1 and q(0, 1, 17) == -1 and q(6, 1, 1) == -1


# ------------------------------------------------------------------ the restatement on hand-made trees
def _drive(worlds, W, E, controls, priors=None, model_of=None):
    """Search hand-made trees: ``worlds[b](path)`` gives the children of the node behind the slots ``path`` as a list of
    ``(q, done)``, at most W.  Every expansion forks the node the restatement named; returns the tree after each expansion
    and the ``parent`` array."""
    B = len(worlds)
    n_cand, q = np.zeros((E, B), np.int64), np.zeros((E, B, W))
    done, parent = np.zeros((E, B, W), bool), np.full((E, B), -1, np.int64)
    pri = np.zeros((E, B, W)) if priors is None else np.broadcast_to(np.asarray(priors, np.float64), (E, B, W))
    paths = [{} for _ in range(B)]
    trees = []
    for t in range(E):
        for b in range(B):
            node = -1 if t == 0 else int(trees[-1].next_node[b])
            if t > 0 and node < 0:
                continue
            parent[t, b] = node
            kids = worlds[b](() if t == 0 else paths[b][node])
            assert len(kids) <= W
            n_cand[t, b] = len(kids)
            for j, (v, d) in enumerate(kids):
                q[t, b, j], done[t, b, j], paths[b][t * W + j] = v, d, (() if t == 0 else paths[b][node]) + (j,)
        rec = search_records(n_cand[:t + 1], pri[:t + 1], q[:t + 1])
        trees.append(search_backup_select(rec, done[:t + 1], parent[:t + 1], controls, model_of, q=q[:t + 1]))
    return trees, parent


def _world(tree):
    """``tree``: a dict path -> children; a path that is not in it has no candidates."""
    return lambda path: tree.get(path, [])


def test_one_expansion_is_the_one_ply_lookahead():
    rng = np.random.default_rng(3)
    B, W = 200, 4
    vl = torch.from_numpy(rng.normal(0, 1.5, (B, W, 3)).astype(np.float32))
    done = torch.from_numpy(rng.random((B, W)) < 0.2)
    rewards = torch.from_numpy(rng.integers(-1, 2, (B, W)).astype(np.float32)) * done
    priors = torch.from_numpy(rng.dirichlet(np.ones(W), B).astype(np.float32))
    n_cand = torch.from_numpy(rng.integers(0, W + 1, B).astype(np.int32))
    q, err = search_leaf_q(vl, rewards, done)
    assert err == 0
    for weight in (0.0, 0.25):                                 # (the table holds the weight in fp32: 0.25 is itself there)
        want = lookahead_choose(priors.double(), n_cand, vl, rewards, done, weight)
        rec = search_records(n_cand[None].numpy(), priors[None].numpy(), q[None].astype(np.float32))
        got = search_backup_select(rec, done[None], np.full((1, B), -1), SearchControls(W, 1, weight), q=q[None])
        assert np.array_equal(got.choice, want.slot.numpy()) and np.array_equal(got.one_ply, got.choice)
        assert np.array_equal(got.u, want.u.numpy()) and not got.deepened.any() and (got.next_node == -1).all()
        used = np.arange(W)[None, :] < n_cand.numpy()[:, None]
        assert np.array_equal(got.val[:, 0][used], want.q.numpy()[used])
    bad = vl.clone()
    bad[0, 0, 1] = float("nan")
    done[0, 0] = False
    q, err = search_leaf_q(bad, rewards, done)
    assert err == ERR_VALUE and np.isneginf(q[0, 0])


def test_a_width_1_chain_with_a_mate_at_depth_3_backs_up_plus_one():
    tree = {(): [(0.0, False)], (0,): [(0.1, False)], (0, 0): [(1.0, True)]}
    trees, parent = _drive([_world(tree)], 1, 4, SearchControls(1, 4))
    assert parent[:, 0].tolist() == [-1, 0, 1, -1]                 # the done node at depth 3 ends the search
    t = trees[2]
    assert t.val[0].reshape(-1).tolist() == [1.0, -1.0, 1.0] and t.finished[0] and t.next_node[0] == -1
    assert trees[3].val[0].reshape(-1).tolist() == [1.0, -1.0, 1.0, 0.0] and trees[3].finished[0]
    assert t.pv[0].tolist() == [0, 1, 2] and t.choice[0] == 0 and not t.deepened[0]
    assert trees[0].next_node[0] == 0 and trees[1].next_node[0] == 1 and trees[1].val[0].reshape(-1).tolist() == [-0.1, 0.1]


def test_a_mate_behind_one_reply_does_not_flip_the_root_while_the_sibling_reply_stands():
    tree = {(): [(0.0, False), (-0.5, False)], (0,): [(0.2, False), (0.1, False)], (0, 0): [(1.0, True), (0.0, False)],
            (0, 1): [(-0.3, False), (-0.4, False)]}
    trees, parent = _drive([_world(tree)], 2, 4, SearchControls(2, 4))
    assert trees[1].val[0, 0].tolist() == [-0.2, -0.5] and trees[1].next_node[0] == 2          # reply a1 is the principal leaf
    t = trees[2]
    assert t.val[0, 1, 0] == -1.0                                  # the reply that allows the mate, at depth 2
    assert t.val[0, 0].tolist() == [-0.1, -0.5] and t.choice[0] == 0                            # the sibling keeps 0.1
    assert t.next_node[0] == 3 and not t.finished[0]               # and is expanded next
    assert parent[:, 0].tolist() == [-1, 0, 2, 3]
    assert trees[3].val[0, 1].tolist() == [-1.0, 0.3] and trees[3].val[0, 0].tolist() == [-0.3, -0.5]
    assert trees[3].pv[0].tolist() == [0, 3, 6, -1] and trees[3].slot[:, 0].tolist() == [0, 1, 0, 0]


def test_a_done_principal_node_finishes_the_search():
    tree = {(): [(1.0, True), (0.5, False)], (1,): [(0.0, False)]}
    trees, parent = _drive([_world(tree)], 2, 3, SearchControls(2, 3))
    assert parent[:, 0].tolist() == [-1, -1, -1] and all(t.finished[0] and t.next_node[0] == -1 for t in trees)
    assert trees[2].choice[0] == 0 and trees[2].pv[0].tolist() == [0, -1, -1] and (trees[2].by[0] == -1).all()


def test_an_expansion_without_candidates_keeps_q_and_finishes():
    tree = {(): [(0.3, False), (0.1, False)]}                      # the principal node has no candidate
    trees, parent = _drive([_world(tree)], 2, 3, SearchControls(2, 3))
    assert parent[:, 0].tolist() == [-1, 0, -1]
    assert trees[1].val[0, 0].tolist() == [0.3, 0.1] and trees[1].by[0, 0].tolist() == [1, -1]
    assert trees[1].finished[0] and trees[1].next_node[0] == -1 and trees[2].choice[0] == 0 and trees[2].slot[1, 0] == -1
    # and a root without candidates is an inactive row
    trees, parent = _drive([_world({})], 2, 2, SearchControls(2, 2))
    assert trees[1].choice[0] == -1 and trees[1].next_node[0] == -1 and not trees[1].finished[0] and (trees[1].pv[0] == -1).all()


def test_ties_take_the_first_maximum_at_the_root_and_below():
    tree = {(): [(0.2, False), (0.2, False), (0.1, False)], (0,): [(-0.2, False), (0.0, False), (0.0, False)],
            (1,): [(-0.2, False)]}
    trees, parent = _drive([_world(tree)], 3, 3, SearchControls(3, 3))
    assert trees[0].choice[0] == 0 and trees[0].next_node[0] == 0
    assert trees[1].slot[1, 0] == 1 and trees[1].val[0, 0].tolist() == [0.0, 0.2, 0.1]           # the first of the two 0.0
    assert trees[1].next_node[0] == 1 and trees[2].val[0, 0].tolist() == [0.0, 0.2, 0.1] and trees[2].choice[0] == 1
    # a prior breaks a root tie only with a weight
    pri = [[[0.1, 0.6, 0.3]]]
    assert _drive([_world(tree)], 3, 1, SearchControls(3, 1, 0.5), pri)[0][0].choice[0] == 1
    assert _drive([_world(tree)], 3, 1, SearchControls(3, 1, 0.0), pri)[0][0].choice[0] == 0


def test_every_model_searches_its_own_expansions():
    tree = {(): [(0.1, False), (0.0, False)], (0,): [(0.5, False)], (1,): [(-0.5, False)], (1, 0): [(0.9, False)]}
    ctl = [SearchControls(2, 3), SearchControls(2, 1), SearchControls(2, 2)]
    trees, parent = _drive([_world(tree)] * 4, 2, 3, ctl, model_of=[0, 1, 2, -1])
    assert parent.T.tolist() == [[-1, 0, 1], [-1, -1, -1], [-1, 0, -1], [-1, -1, -1]]
    t = trees[2]
    assert t.choice.tolist() == [1, 0, 1, 0] and t.deepened.tolist() == [True, False, True, False]
    assert t.val[0, 0].tolist() == [-0.5, 0.5] and t.val[2, 0].tolist() == [-0.5, 0.0] and t.val[1, 0].tolist() == [0.1, 0.0]
    assert t.pv.tolist() == [[1, 4, -1], [0, -1, -1], [1, -1, -1], [0, -1, -1]]
    assert trees[0].next_node.tolist() == [0, -1, 0, -1] and trees[1].next_node.tolist() == [1, -1, -1, -1]


def test_the_sign_of_the_backup_and_the_max_decide_these_trees():
    # with val(n) = + max the reply that is good for the opponent would speak for the move: the choice would stay 0
    sign = {(): [(0.1, False), (0.0, False)], (0,): [(0.5, False)]}
    t = _drive([_world(sign)], 2, 2, SearchControls(2, 2))[0][1]
    assert t.val[0, 0].tolist() == [-0.5, 0.0] and t.choice[0] == 1 and t.deepened[0]
    # with min in the place of max the opponent would pick the worst reply: val would be +0.5 and the choice would stay 0
    minmax = {(): [(0.1, False), (0.0, False)], (0,): [(0.5, False), (-0.5, False)]}
    t = _drive([_world(minmax)], 2, 2, SearchControls(2, 2))[0][1]
    assert t.val[0, 0].tolist() == [-0.5, 0.0] and t.choice[0] == 1 and t.slot[1, 0] == 0


def test_the_shared_table_reader_field_checks_and_the_one_place_rule():
    from test_lookahead_cpu import check_field_refusals, check_table_of
    check_table_of(search_table, "search", SearchControls(3, 4, 0.25), [SearchControls(3, 4, 0.25, 2), SearchControls()])
    check_field_refusals(lambda **kw: SearchControls(**dict({"width": 1}, **kw)),
                         ints=(("width", 8), ("skip_plies", 65535), ("expansions", MAX_EXPANSIONS)), weights=("prior_weight",))
    # stated once, over the stage list: refused before the ply touches a device
    from keisei_amd.training._device_ply import DevicePly
    from keisei_amd.training.lookahead import LookaheadStage
    from keisei_amd.training.mcts_search import MctsControls, MctsStage
    from keisei_amd.training.tree_search import SearchStage
    la, se, mc = (LookaheadStage.parse(LookaheadControls(2), 2, False), SearchStage.parse(SearchControls(2, 2), 2, False),
                  MctsStage.parse(MctsControls(2, 2), 2, False))
    for stages, text in (((la, se), "search= cannot be combined with lookahead="), ((se, mc), "mcts= cannot be combined with search="),
                         ((la, None, mc), "mcts= cannot be combined with lookahead=")):
        with pytest.raises(ValueError, match=text):
            DevicePly(None, 16, 24, stages=stages)
    assert (la.sizes, se.sizes, mc.sizes) == (dict(width=2, reply_width=0), dict(width=2, expansions=2), dict(width=2, simulations=2))
    assert la.engine is None and la.table is None and LookaheadStage.parse(None, 2, False) is None
