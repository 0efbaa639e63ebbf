"""The arena's ply, launch for launch: every option's docstring promises that a ply without the option is "launch for
launch what it was".  Each configuration below is built, its ply is run twice and the names that went through
``_lib.call`` are compared with a literal list, taken from the commit before the searches were folded into one stage list.
The grouped forward binds ``_lib.call`` at import (``keisei_amd.hip.group._call``), so that name is wrapped too; every run of
names outside the ply's own prefixes is one ``"forward"``."""
import pytest
import torch

import keisei_amd.hip.group as hip_group
from keisei_amd import _lib
from keisei_amd.training import (LookaheadControls, MatchArena, MateControls, MctsControls, MctsExploration, SamplingControls,
                                 SearchControls)
from test_hip_lookahead_replies import MAX_PLY, N, PER, _group

pytestmark = pytest.mark.gpu

KEPT = ("ka_policy_sample", "ka_policy_insight", "ka_lookahead_", "ka_search_", "ka_mcts_", "ka_mate", "ka_shogi_env_step",
        "ka_spectator_", "ka_gamelog_", "ka_arena_")
F, STEP = "forward", "ka_shogi_env_step"

PLAIN = [F, "ka_policy_sample_play", STEP, "ka_arena_referee"]
MATE1 = ["ka_mate_fork", STEP, "ka_mate_choose"]
EXPECTED = {
    "plain": PLAIN,
    "lookahead_mate_insight_log": [
        F, "ka_policy_sample_ctl", "ka_lookahead_fork", STEP, F, "ka_lookahead_fork_replies", STEP, F,
        "ka_lookahead_choose_replies", *MATE1, "ka_policy_insight", STEP, "ka_gamelog_step", "ka_arena_referee"],
    "search_mate3_features": [
        F, "ka_policy_sample_play",
        "ka_lookahead_fork", STEP, F, "ka_search_advance",
        *(["ka_search_expand", STEP, F, "ka_search_advance"] * 3),
        *MATE1, "ka_mate3_fork", STEP, "ka_mate3_gate", *MATE1, "ka_mate3_choose",
        STEP, "ka_arena_features_step", "ka_arena_referee"],
    "mcts_explore_samples_log": [
        F, "ka_policy_sample_play",
        "ka_lookahead_fork", "ka_mcts_root_noise", STEP, F, "ka_mcts_advance_explore",
        *(["ka_search_expand", STEP, F, "ka_mcts_advance_explore"] * 2),
        STEP, "ka_search_sample_step", "ka_gamelog_step", "ka_arena_referee"],
    "everything_off": PLAIN,
}
CONFIGS = {
    "plain": {},
    "lookahead_mate_insight_log": dict(sampling=SamplingControls(temperature=0.8, top_k=4),
                                       lookahead=[LookaheadControls(3, 0.25, reply_width=2), LookaheadControls.OFF],
                                       mate=MateControls(4), insight=3, game_log=64),
    "search_mate3_features": dict(search=SearchControls(3, 4), mate=MateControls(4, 0, 8, 2), features=True),
    "mcts_explore_samples_log": dict(mcts=MctsControls(3, 3, 1.25), mcts_explore=MctsExploration(0.25, 0.3, 8),
                                     search_samples=8, game_log=64),
    "everything_off": dict(lookahead=LookaheadControls.OFF, search=None, mate=MateControls.OFF),
}


def _collapse(names):
    out = []
    for n in names:
        n = n if n.startswith(KEPT) else F
        if n != F or out[-1:] != [F]:
            out.append(n)
    return out


def _launches(monkeypatch, **options):
    arena = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=False, seed=23, **options)
    arena.ply.reset()
    names, call = [], _lib.call

    def noting(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", noting)
    monkeypatch.setattr(hip_group, "_call", noting)
    plies = []
    with torch.no_grad():
        for _ in range(2):
            del names[:]
            arena._ply()
            plies.append(_collapse(names))
    monkeypatch.undo()
    torch.cuda.synchronize()
    return plies


@pytest.mark.parametrize("config", list(CONFIGS))
def test_the_ply_launches_what_it_launched(config, monkeypatch):
    first, second = _launches(monkeypatch, **CONFIGS[config])
    print(f"\n{config}: {first}")
    assert first == second
    assert first == EXPECTED[config]
