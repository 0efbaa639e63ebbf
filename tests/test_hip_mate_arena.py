"""MatchArena(mate=): games started from mate-in-one positions are won at once by the model that has the mate check, under
a captured graph as without one; an all-off table changes nothing; set_mate() switches the behaviour between rounds."""
import gc

import pytest
import torch

import mate_search_helpers as H
from keisei_amd.training import MatchArena, MateControls
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)             # the smallest group the kernels accept: 128 channels, 2 blocks
N, PER, MAX_PLY = 8, 4, 40
PAIRINGS = [(0, 1), (1, 0)]
ON = [MateControls(16), MateControls.OFF]                    # model 0 alone looks for mates
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
    arena.env.set_start_sfens(H.pool_sfens(), seed=5)         # every game starts from a mate in one, for either colour
    return arena


def _key(results):
    return [(r.a, r.b, r.a_wins, r.b_wins, r.draws, r.plies, r.partial) for r in results]


def _games(results):
    return [[(g.env, g.start_sfen(), g.winner, g.reason, g.end_ply, tuple(int(a) for a in g.actions)) for g in r.recorded_games]
            for r in results]


def _first_mover(g):
    return g.black if g.start_side == 0 else g.white


def _won_at_once(results):
    """The games model 0 moved first in, all of which must be one ply long and won by checkmate; returns their count."""
    count = 0
    for r in results:
        for g in r.recorded_games:
            if g.carried or _first_mover(g) != 0:
                continue
            count += 1
            assert len(g.actions) == 1 and g.reason == CHECKMATE and g.winner == g.start_side and not g.truncated, \
                (g.env, g.start_sfen(), g.actions, g.reason, g.winner)
    return count


def test_model_zero_mates_at_once_and_graph_equals_eager():
    eager, graph = _arena(False, ON), _arena(True, ON)
    r1, s1 = eager.run_round(PAIRINGS, games_per_match=8)
    r2, s2 = graph.run_round(PAIRINGS, games_per_match=8)
    assert graph._graph is not None and eager._graph is None and eager.ply.stages["mate"].mate.cap == 16
    count = _won_at_once(r1)
    assert count >= 4 and s1.mate.mates >= count and s1.mate.positions >= s1.mate.mates and s1.games_dropped == 0
    assert s1.mate.forked >= s1.mate.positions and s1.mate.changed <= s1.mate.mates
    # the games model 1 moved first in are not all over at once: it has no mate check
    slow = [g for r in r1 for g in r.recorded_games if not g.carried and _first_mover(g) == 1]
    assert slow and any(len(g.actions) > 1 for g in slow)
    assert _key(r1) == _key(r2) and _games(r1) == _games(r2) and s1.round_plies == s2.round_plies
    assert s1.mate == s2.mate and torch.equal(eager.ply.stages["mate"].mate.records(), graph.ply.stages["mate"].mate.records())


def test_an_all_off_table_is_the_plain_arena_and_set_mate_switches_between_rounds():
    plain, arena = _arena(True, None), _arena(True, ON)
    assert "mate" not in plain.ply.stages
    r0, s0 = plain.run_round(PAIRINGS, games_per_match=8)
    r_on, s_on = arena.run_round(PAIRINGS, games_per_match=8)
    graph = arena._graph
    assert s0.mate is None and s_on.mate.mates > 0 and _games(r_on) != _games(r0)
    arena.set_mate(None)                                      # the launches stay in the ply, every row is off
    r1, s1 = arena.run_round(PAIRINGS, games_per_match=8)
    assert s1.mate == type(s1.mate)() and _key(r1) == _key(r0) and _games(r1) == _games(r0) and s1.round_plies == s0.round_plies
    assert sum(len(g) for g in _games(r0)) >= 8
    arena.set_mate({0: MateControls(16)})                     # on again, under the same captured graph
    r2, s2 = arena.run_round(PAIRINGS, games_per_match=8)
    assert arena._graph is graph and _key(r2) == _key(r_on) and _games(r2) == _games(r_on) and s2.mate == s_on.mate
    assert _won_at_once(r2) >= 4
    # built with every row off: nothing is allocated and nothing is launched, and nothing can be switched on later
    idle = _arena(True, MateControls.OFF)
    assert idle.ply.stages["mate"].mate is None and idle.ply.stages["mate"].table is not None
    r3, s3 = idle.run_round(PAIRINGS, games_per_match=8)
    assert _key(r3) == _key(r0) and _games(r3) == _games(r0) and s3.mate == type(s3.mate)()
    with pytest.raises(ValueError, match="above the largest"):
        idle.set_mate(MateControls(1))


def test_refusals():
    with pytest.raises(ValueError, match="collect=True"):
        MatchArena(_group(), N, PER, MAX_PLY, collect=True, mate=MateControls())
    arena = MatchArena(_group(), N, PER, MAX_PLY, graph=False, mate=MateControls(4))
    with pytest.raises(ValueError, match="above the largest"):
        arena.set_mate(MateControls(5))
    with pytest.raises(ValueError, match="expected 2"):
        arena.set_mate([MateControls()])
    plain = MatchArena(_group(), N, PER, MAX_PLY, graph=False)
    with pytest.raises(ValueError, match="built without mate"):
        plain.set_mate(MateControls.OFF)
