"""MatchArena(mate=) with evasion_rows > 0: games started from mate-in-three positions are won in three plies by the model
that has the deeper check, whatever the other model replies, under a captured graph as without one; a table with
evasion_rows 0 plays the games of the mate-in-one arena; set_mate() switches depth three on and off between rounds."""
import gc

import pytest
import torch

import mate3_helpers as M
from keisei_amd.training import MatchArena, MateControls
from keisei_amd.training.mate_search import Mate3Stats
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)             # the smallest group the kernels accept: 128 channels, 2 blocks
N, PER, MAX_PLY = 8, 4, 40
PAIRINGS = [(0, 1), (1, 0)]
DEEP = [MateControls(*M.POOL_CAPS[:1], 0, *M.POOL_CAPS[1:]), MateControls.OFF]      # model 0 alone looks for mates, three deep
ONE = [MateControls(16), MateControls.OFF]                   # the mate in one alone
CHECKMATE = 1
_GROUP = []


@pytest.fixture(autouse=True)
def _release_device_objects():
    """Arenas own captured graphs and pinned buffers: collect them with the device idle, not inside a later test's
    capture (tests/test_hip_league_rollout.py)."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _group():
    if not _GROUP:
        models = []
        for k in range(2):
            m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
            m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=31 * k + 7), strict=True)
            models.append(m.to(DEV).eval())
        _GROUP.append(SEResNetGroup(models))
    return _GROUP[0]


def _arena(graph, mate, seed=17, **kw):
    arena = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=graph, seed=seed, game_log=256,
                       start_pool_capacity=16, mate=mate, **kw)
    arena.env.set_start_sfens(M.pool_sfens(), seed=5)         # every game starts from a mate in three, for either colour
    return arena


def _key(results):
    return [(r.a, r.b, r.a_wins, r.b_wins, r.draws, r.plies, r.partial) for r in results]


def _games(results):
    return [[(g.env, g.start_sfen(), g.winner, g.reason, g.end_ply, tuple(int(a) for a in g.actions)) for g in r.recorded_games]
            for r in results]


def _first_mover(g):
    return g.black if g.start_side == 0 else g.white


def _won_in_three(results):
    """The games model 0 moved first in, all of which must be three plies long and won by checkmate; returns their count."""
    count = 0
    for r in results:
        for g in r.recorded_games:
            if g.carried or _first_mover(g) != 0:
                continue
            count += 1
            assert len(g.actions) == 3 and g.reason == CHECKMATE and g.winner == g.start_side and not g.truncated, \
                (g.env, g.start_sfen(), g.actions, g.reason, g.winner)
    return count


def test_model_zero_mates_in_three_and_graph_equals_eager():
    eager, graph = _arena(False, DEEP, record=True), _arena(True, DEEP)
    r1, s1 = eager.run_round(PAIRINGS, games_per_match=8)
    r2, s2 = graph.run_round(PAIRINGS, games_per_match=8)
    assert graph._graph is not None and eager._graph is None
    assert (eager.ply.stages["mate"].mate.cap, eager.ply.stages["mate"].mate3.rows, eager.ply.stages["mate"].mate3.reply_cap) == M.POOL_CAPS and eager.ply.stages["mate"].mate3.root is eager.ply.stages["mate"].mate
    count = _won_in_three(r1)
    assert count >= 4 and s1.mate3.mates >= count and s1.mate.mates >= count and s1.games_dropped == 0
    assert s1.mate3.positions >= s1.mate3.mates >= s1.mate3.changed and s1.mate3.rows >= s1.mate3.positions
    assert s1.mate3.reply_rows >= s1.mate3.rows
    # the games model 1 moved first in are not all over in three: it has no mate check
    slow = [g for r in r1 for g in r.recorded_games if not g.carried and _first_mover(g) == 1]
    assert slow and any(len(g.actions) != 3 or g.reason != CHECKMATE for g in slow)
    assert _key(r1) == _key(r2) and _games(r1) == _games(r2) and s1.round_plies == s2.round_plies
    assert s1.mate == s2.mate and s1.mate3 == s2.mate3
    assert torch.equal(eager.ply.stages["mate"].mate.records(), graph.ply.stages["mate"].mate.records()) and torch.equal(eager.ply.stages["mate"].mate3.records(), graph.ply.stages["mate"].mate3.records())
    assert all("mate3_records" in rec and rec["mate3_records"].shape == (N, 6 + 2 * 16) for rec in eager.record)


def test_evasion_rows_zero_is_the_mate_in_one_arena_and_set_mate_switches_between_rounds():
    one, arena = _arena(True, ONE), _arena(True, DEEP)
    assert one.ply.stages["mate"].mate3 is None and one.ply.stages["mate"].reply_table is None and one.ply.stages["mate"].mate is not None
    r0, s0 = one.run_round(PAIRINGS, games_per_match=8)
    r_on, s_on = arena.run_round(PAIRINGS, games_per_match=8)
    graph = arena._graph
    assert s0.mate3 is None and s_on.mate3.mates > 0 and _games(r_on) != _games(r0)
    arena.set_mate(ONE)                                       # the launches stay in the ply, depth three is off in every row
    r1, s1 = arena.run_round(PAIRINGS, games_per_match=8)
    assert s1.mate3 == Mate3Stats() and s1.mate == s0.mate
    assert _key(r1) == _key(r0) and _games(r1) == _games(r0) and s1.round_plies == s0.round_plies
    assert sum(len(g) for g in _games(r0)) >= 8
    arena.set_mate({0: DEEP[0]})                              # on again, under the same captured graph
    r2, s2 = arena.run_round(PAIRINGS, games_per_match=8)
    assert arena._graph is graph and _key(r2) == _key(r_on) and _games(r2) == _games(r_on)
    assert s2.mate == s_on.mate and s2.mate3 == s_on.mate3 and _won_in_three(r2) >= 4


def test_refusals():
    with pytest.raises(ValueError, match="collect=True"):
        MatchArena(_group(), N, PER, MAX_PLY, collect=True, mate=MateControls(16, 0, 32, 8))
    arena = MatchArena(_group(), N, PER, MAX_PLY, graph=False, mate=MateControls(4, 0, 8, 2))
    for controls, text in ((MateControls(5, 0, 8, 2), "max_checks 5"), (MateControls(4, 0, 9, 2), "evasion_rows 9"),
                           (MateControls(4, 0, 8, 3), "reply_checks 3")):
        with pytest.raises(ValueError, match=f"{text} is above the largest"):
            arena.set_mate(controls)
    arena.set_mate(MateControls(4, 0, 8, 1))
    assert arena.ply.stages["mate"].table.tolist() == [[4, 0, 8, 1]] * 2 and arena.ply.stages["mate"].reply_table.tolist() == [[1, 0, 0, 0]] * 2
    one = MatchArena(_group(), N, PER, MAX_PLY, graph=False, mate=MateControls(4))
    with pytest.raises(ValueError, match="evasion_rows 1 is above the largest"):
        one.set_mate(MateControls(4, 0, 1, 1))
