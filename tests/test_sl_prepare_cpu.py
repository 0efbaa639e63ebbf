"""CPU tests of keisei_amd.sl.parsers / keisei_amd.sl.prepare (SL shard preparation) against tests/golden/g15_*:
the parsers against the reference parsers' recorded output, ``usi_to_action`` against the oracle's encoder, the host
restatement ``_replay_host`` over the CPU env oracle against the fixture's one-game-at-a-time replay, and the file handling
of ``prepare_sl_data`` with that host replay in the device's place.  Every comparison is exact."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, SpatialActionMapper
from keisei_amd.sl import prepare as prep
from keisei_amd.sl.dataset import OBS_SIZE, RECORD_SIZE, SLDataset
from keisei_amd.sl.parsers import CSAParser, GameFilter, GameOutcome, GameRecord, ParsedMove, SFENParser, is_standard_start
from oracle import shogi as so
from sl_prepare_helpers import (FILES, GOLDEN, RANKS, check_against_golden, fixture_games, oracle_replay, parsed_records,
                                shifted_observations)


# ------------------------------------------------------------------ parsers
def test_parsers_equal_the_reference_parsers_output(golden):
    g = golden("g15_sl_prepare")
    recs = parsed_records()
    off = g.np("move_offsets")
    assert len(recs) == len(g.np("outcomes")) == len(off) - 1
    per_file = [len(list(SFENParser().parse(FILES[0]))), len(list(CSAParser().parse(FILES[1])))]
    assert per_file == np.bincount(g.np("file_of"), minlength=2).tolist()
    for k, rec in enumerate(recs):
        assert [m.move_usi for m in rec.moves] == g.np("moves")[off[k]:off[k + 1]].tolist(), g.np("tags")[k]
        assert all(m.sfen_before == "" for m in rec.moves)
        assert rec.outcome.value == str(g.np("outcomes")[k])
        sel = g.np("meta_game") == k
        assert rec.metadata == dict(zip(g.np("meta_keys")[sel].tolist(), g.np("meta_vals")[sel].tolist())), g.np("tags")[k]
        assert is_standard_start(rec.start) == bool(g.np("standard_start")[k]), (g.np("tags")[k], rec.start)
    assert {r.outcome for r in recs} == set(GameOutcome)
    assert SFENParser().supported_extensions() == {".sfen"} and CSAParser().supported_extensions() == {".csa"}


def test_parser_record_semantics(tmp_path):
    p = tmp_path / "a.sfen"
    p.write_text("result:win_black\r\nrating: 1800\r\nstartpos\r\n7g7f\r\n\r\nresult:nobody\nstartpos\n7g7f\n\n"
                 "result:draw\nstartpos\n\nresult:win_white\nlnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b - 1\n3c3d\n")
    recs = list(SFENParser().parse(p))
    assert [(len(r.moves), r.outcome) for r in recs] == [(1, GameOutcome.WIN_BLACK), (1, GameOutcome.WIN_WHITE)]
    assert recs[0].metadata == {"result": "win_black", "rating": "1800"} and recs[0].start == "startpos"
    assert is_standard_start(recs[1].start) and not is_standard_start("lnsgkgsnl/9/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b - 1")
    c = tmp_path / "b.csa"
    c.write_text("V2.2\nN+a\nN-b\n$EVENT:x\nPI\n+\n+7776FU\n-3334FU\n+8822UM\n%TORYO\n/\nPI\n+\n+7776FU\n-33\n%TORYO\n/\n"
                 "PI\n+\n+7776FU\n%CHUDAN\n/\nPI\n+\n+7770FU\n%TORYO\n/\nPI82HI\n+\n+7776FU\n-0055KA\n+%TORYO\n")
    recs = list(CSAParser().parse(c))
    assert [[m.move_usi for m in r.moves] for r in recs] == [["7g7f", "3c3d", "8h2b+"], ["7g7f", "B*5e"]]
    assert recs[0].outcome == GameOutcome.WIN_BLACK and recs[0].metadata == {"player_black": "a", "player_white": "b", "event": "x"}
    assert recs[1].outcome == GameOutcome.WIN_WHITE                     # "+%TORYO": black resigns, the last mover wins
    assert recs[0].start == "startpos" and not is_standard_start(recs[1].start)
    rec = GameRecord([ParsedMove("7g7f")] * 3, GameOutcome.DRAW, {"black_rating": "1500", "white_rating": "x"})
    assert GameFilter(min_ply=3).accepts(rec) and not GameFilter(min_ply=4).accepts(rec)
    assert GameFilter(min_ply=1, min_rating=1500).accepts(rec) and not GameFilter(min_ply=1, min_rating=1501).accepts(rec)


# ------------------------------------------------------------------ USI -> action
def _usi(frm, to, promote, drop):
    sq = lambda s: f"{9 - s % 9}{RANKS[s // 9]}"  # noqa: E731
    return f"{'?PLNSGBR'[drop]}*{sq(to)}" if drop else sq(frm) + sq(to) + ("+" if promote else "")


def test_usi_to_action_equals_the_oracle_encoder_and_inverts():
    mapper, kinds = SpatialActionMapper(), set()
    for white in (False, True):
        for idx in range(ACTION_SPACE):
            d = so.decode(idx, white)
            if d is None:
                continue
            frm, to, promote, drop = d
            assert so.encode(frm, to, bool(promote), drop, white) == idx
            assert prep.usi_to_action(_usi(*d), white) == idx, (idx, white, d)
            back = mapper.decode(idx, white)
            if drop:
                assert back == {"type": "drop", "to_sq": to, "piece_type_idx": drop - 1}
            else:
                assert back == {"type": "board", "from_sq": frm, "to_sq": to, "promote": bool(promote)}
            slot = idx % 139
            kinds.add(("drop" if drop else "knight" if slot >= 128 else "slide", bool(promote), white))
    assert len(kinds) == 10                                      # drops, knight and sliding moves with and without promotion, both colours
    assert prep.usi_to_action("7g7f", False) == prep.usi_to_action("3c3d", True)      # the mover's perspective
    for bad in ("", "resign", "7g7", "7g7f++", "0a1b", "5j5i", "K*5e", "p*5e", "P*0e", "5i3f", "8b5a", "5e5e", "8i7g+x"):
        with pytest.raises(ValueError):
            prep.usi_to_action(bad, False)
    with pytest.raises(ValueError):
        prep.usi_to_action("7g8i", False)                        # a knight's jump backwards: no plane holds it
    assert prep.usi_to_action("7g8i", True) == prep.usi_to_action("3c2a", False)


def test_encode_game_cuts_where_the_text_cannot_be_encoded():
    rec = GameRecord([ParsedMove(m) for m in ("7g7f", "3c3d", "oops", "2g2f")], GameOutcome.DRAW)
    a, why = prep._encode_game(rec, 10)
    assert a.tolist() == [prep.usi_to_action("7g7f", False), prep.usi_to_action("3c3d", True)] and why == prep.REASON_NO_ENCODING
    a, why = prep._encode_game(rec, 2)
    assert len(a) == 2 and why == prep.REASON_LONG


# ------------------------------------------------------------------ the host restatement against the fixture
@pytest.fixture(scope="module")
def host_replay(golden):
    g = golden("g15_sl_prepare")
    games, index = fixture_games(g)
    batch = prep.ReplayBatch.build(games)
    out = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, int(g.np("max_moves"))))
    return g, games, index, batch, out


def test_replay_host_reproduces_the_golden_replay(host_replay):
    g, games, index, batch, (buf, valid_len, reason, hdr) = host_replay
    assert batch.rows == sum(len(a) for a, _, _ in games) and sorted(batch.order.tolist()) == list(range(len(games)))
    assert (np.diff(batch.length) <= 0).all()                   # slots sorted by length, rows in record order
    check_against_golden(g, games, index, batch, buf, valid_len, reason)
    assert int(valid_len.sum()) == len(g.np("pos_policy")) == int(hdr[prep._WRITTEN])
    assert int(hdr[prep._ILLEGAL]) == int((g.np("reason") == 1).sum()) and int(hdr[prep._RULES]) == int(g.np("games_cut_by_rules"))
    assert int(hdr[prep._PLIES]) == int(batch.length.max()) and int(hdr[prep._STALL]) == 0
    assert int(hdr[prep._WRITTEN] + hdr[prep._FILLER]) == int(hdr[prep._PLIES]) * batch.num_envs
    tags = g.np("tags").tolist()
    assert {tags[index[k]]: int(len(games[k][0])) for k in range(len(games))}["plain1"] == 1
    assert (buf["value"][prep._kept_rows(batch, valid_len)] <= 2).all()
    assert set(np.unique(g.np("pos_value")).tolist()) == {0, 1, 2}


def test_a_flipped_value_or_a_late_observation_fails_the_comparison(host_replay, monkeypatch):
    g, games, index, batch, _ = host_replay
    env = lambda: so.OracleVecEnv(batch.num_envs, int(g.np("max_moves")))  # noqa: E731
    with monkeypatch.context() as m:
        m.setattr(prep, "_value_of", lambda outcome, mover: 1 if outcome == 2 else (2 if outcome == mover else 0))
        buf, valid_len, reason, _ = prep._replay_host(batch, env())
        with pytest.raises(AssertionError):
            check_against_golden(g, games, index, batch, buf, valid_len, reason)
    buf, valid_len, reason, _ = prep._replay_host(batch, env())
    check_against_golden(g, games, index, batch, buf, valid_len, reason)
    late = shifted_observations(batch, buf, valid_len)           # every record with the observation AFTER its move
    with pytest.raises(AssertionError):
        check_against_golden(g, games, index, batch, late, valid_len, reason)


def test_batches_respect_both_caps(golden):
    games, _ = fixture_games(golden("g15_sl_prepare"))
    for envs, cap in ((5, 10 ** 6), (64, 150), (1, 96)):
        got = list(prep._batches(iter(games), envs, cap))
        assert [x for b in got for x in b] == games
        assert all(len(b) <= envs and (sum(len(x[0]) for x in b) <= cap or len(b) == 1) for b in got)
    padded = prep.ReplayBatch.build(games[:3]).padded(8)
    assert padded.num_envs == 8 and padded.length[3:].tolist() == [0] * 5 and padded.order[3:].tolist() == [-1] * 5


# ------------------------------------------------------------------ files
def test_prepare_files_with_the_host_replay(golden, tmp_path):
    """shard_size = 7 falls inside games; SLDataset reads the directory without allow_placeholder; a second, smaller run
    leaves no stale shard."""
    g = golden("g15_sl_prepare")
    max_moves = 20
    out = tmp_path / "shards"
    meta = prep._prepare([str(GOLDEN)], str(out), GameFilter(min_ply=1), 7, oracle_replay(max_moves), batch_envs=8,
                         max_moves=max_moves, max_batch_positions=100)
    games, index = fixture_games(g, max_moves)
    batch = prep.ReplayBatch.build(games)
    buf, valid_len, reason, _ = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, max_moves))
    want = buf[prep._kept_rows(batch, valid_len)]
    n = len(want)
    shards = sorted(out.glob("shard_*.bin"))
    assert [s.name for s in shards] == [f"shard_{k:03d}.bin" for k in range((n + 6) // 7)]
    assert [s.stat().st_size for s in shards] == [7 * RECORD_SIZE] * (n // 7) + ([n % 7 * RECORD_SIZE] if n % 7 else [])
    assert b"".join(s.read_bytes() for s in shards) == want.tobytes()
    assert 0 < int(valid_len[0]) % 7 or 0 < int(valid_len[:2].sum()) % 7       # a shard boundary inside a game
    assert json.loads((out / "shard_meta.json").read_text()) == meta
    final = np.where(reason != 0, reason, np.array([x[2] for x in games])[batch.order])
    assert meta == {"placeholder": False, "num_shards": len(shards), "num_games": len(games), "num_positions": n,
                    "games_cut_illegal": int(((final == 1) | (final == 4)).sum()), "games_cut_by_rules": int((final == 2).sum()),
                    "games_cut_long": sum(len(r.moves) > max_moves for r in parsed_records() if is_standard_start(r.start)),
                    "games_nonstandard_start": int(g.np("games_nonstandard_start"))}
    assert meta["games_cut_long"] > 2 and meta["games_cut_illegal"] >= 3
    ds = SLDataset(out)                                          # placeholder: false -- no allow_placeholder needed
    assert len(ds) == n
    got = ds.read_batch(np.arange(n))
    assert torch.equal(got["observation"].reshape(n, OBS_SIZE), torch.from_numpy(want["obs"].copy()))
    assert torch.equal(got["policy_target"], torch.from_numpy(want["policy"].copy()))
    assert torch.equal(got["value_target"], torch.from_numpy(want["value"].copy()))
    assert torch.equal(got["score_target"], torch.from_numpy(want["score"].copy()))
    item = ds[n - 1]
    assert item["observation"].shape == (50, 9, 9) and int(item["policy_target"]) == int(want["policy"][-1])
    # a second run with fewer games: every shard of the first run that it does not rewrite is gone
    (out / "shard_900.bin").write_bytes(b"\0" * RECORD_SIZE)
    meta2 = prep._prepare([str(FILES[0])], str(out), GameFilter(min_ply=30), 7, oracle_replay(max_moves), batch_envs=8,
                          max_moves=max_moves, max_batch_positions=100)
    assert 0 < meta2["num_games"] < meta["num_games"] and meta2["num_shards"] < meta["num_shards"]
    assert len(list(out.glob("shard_*.bin"))) == meta2["num_shards"] and len(SLDataset(out)) == meta2["num_positions"]
    assert not list(out.glob("*.tmp"))


def test_a_bad_record_or_file_does_not_lose_the_rest(tmp_path):
    class Flaky(SFENParser):
        def parse(self, path):
            yield "first"
            raise RuntimeError("broken record")

    class Closed(SFENParser):
        def parse(self, path):
            raise OSError("unreadable")

    assert list(prep._records_of(Flaky(), tmp_path / "x.sfen")) == ["first", None]
    assert list(prep._records_of(Closed(), tmp_path / "x.sfen")) == [None]
    (tmp_path / "a.sfen").write_text("x")
    (tmp_path / "B.CSA").write_text("x")
    (tmp_path / "c.txt").write_text("x")
    found = prep._discover([str(tmp_path), str(tmp_path / "c.txt"), str(tmp_path / "none")], prep._parsers_by_extension())
    assert [f.name for f in found] == ["a.sfen", "B.CSA", "c.txt"]


def test_prepare_needs_a_gpu_and_touches_nothing_without_one(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    out = tmp_path / "o"
    out.mkdir()
    (out / "shard_000.bin").write_bytes(b"\0" * RECORD_SIZE)
    with pytest.raises(_lib.KeiseiHipError):
        prep.prepare_sl_data([str(GOLDEN)], str(out), min_ply=1)
    with pytest.raises(ValueError, match="max_moves"):            # the env counts plies in 16 bits
        prep.prepare_sl_data([str(GOLDEN)], str(out), min_ply=1, max_moves=65536)
    assert (out / "shard_000.bin").exists()
    import sys
    assert "oracle" not in prep.__dict__ and not any("oracle" in str(getattr(v, "__module__", "")) for v in prep.__dict__.values())
    assert sys.modules["keisei_amd.sl.prepare"] is prep
