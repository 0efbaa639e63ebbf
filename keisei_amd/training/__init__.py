"""Host-side mirror of the reference's ``keisei.training`` hot-path API (same names, arguments,
error behaviour), backed by hand-written HIP kernels for GPU tensors."""
from .dynamic_trainer import DynamicTrainer, MatchRollout  # noqa: F401
from .game_log import GameLog, RecordedGame, game_log_host, write_sfen_games  # noqa: F401
from .game_feature_tracker import GameFeatureAccumulator, GameFeatureRow, GameFeatureTracker, classify_action  # noqa: F401
from .league_rollout import LeagueRollout, LeagueRolloutStats  # noqa: F401
from .lookahead import (Lookahead, LookaheadChoice, LookaheadControls, LookaheadReplyChoice, LookaheadStats,  # noqa: F401
                        lookahead_active, lookahead_candidates, lookahead_choose, lookahead_choose_replies,
                        lookahead_reply_widths, lookahead_table)
from .mate_search import Mate3Search, Mate3Stats, MateControls, MateSearch, MateStats, mate_table  # noqa: F401
from .match_arena import MatchArena, MatchResult, RoundStats  # noqa: F401
from .mcts_explore import MctsExploration, explore_table, root_noise_host, visit_choice_host  # noqa: F401
from .mcts_search import (MctsControls, MctsRestatement, MctsSearch, MctsStats, MctsTree, mcts_backup_select,  # noqa: F401
                          mcts_simulations, mcts_table, visit_policy)
from .policy_insight import InsightRecorder, PolicyInsight, action_usi, insight_dict, policy_insight  # noqa: F401
from .sampling import ControlledSample, SamplingControls, controls_table, sample_controlled  # noqa: F401
from .search_samples import (SearchSamples, SearchSampleStats, search_sample_step_host, unpack_visit_words,  # noqa: F401
                             visit_words)
from .selfplay_rollout import SelfPlayRollout, SelfPlayStats  # noqa: F401
from .tree_search import (SearchControls, SearchStats, SearchTree, TreeSearch, search_backup_select,  # noqa: F401
                          search_expansions, search_leaf_q, search_records, search_table)
