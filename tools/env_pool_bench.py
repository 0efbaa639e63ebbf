"""Time of one env step (clear + validate + shogi_env_kernel, HIP events around the three launches) of a given build of
the library, without and with a pool of start positions: katago / spatial, random legal play, 128 and 16 384 games.

    python tools/env_pool_bench.py <libkeisei_amd.so> [label]

Talks to the C ABI through ctypes and not through keisei_amd._lib, so that a build from before the pool entry points can
be timed by the same code (it then reports the path without a pool only).  One JSON line per case.  To compare two
builds, alternate them inside one job (tools/ab_bench.sh does that for bench.py) and take the older build's run-to-run
difference as the margin."""
import ctypes
import json
import sys

import torch

path, label = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else sys.argv[1])
lib = ctypes.CDLL(path)
has_pool = hasattr(lib, "ka_shogi_env_step_pool")
A, C, MAX_PLY, WARM, STEPS = 81 * 139, 50, 64, 30, 300        # max_ply 64: every game restarts a few times
P = ctypes.c_void_p
p = lambda t: P(t.data_ptr()) if t is not None else P(None)  # noqa: E731


def run(n: int, pooled: bool) -> dict:
    z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device="cuda")  # noqa: E731
    state, keys, checks = z(n, 128, dtype=torch.uint8), z(n, MAX_PLY, dtype=torch.int64), z(n, MAX_PLY, dtype=torch.uint8)
    obs = [z(n, C, 9, 9, dtype=torch.float32) for _ in range(2)]
    mask = [z(n, A, dtype=torch.bool) for _ in range(2)]
    bits = [z(n, (A + 31) // 32, dtype=torch.int32) for _ in range(2)]
    players, rewards = z(n, dtype=torch.uint8), z(n, dtype=torch.float32)
    term, trunc, cap, reason = (z(n, dtype=torch.uint8) for _ in range(4))
    ply, material, tobs = z(n, dtype=torch.int16), z(n, dtype=torch.int32), z(n, C, 9, 9, dtype=torch.float32)
    stats, err = z(4, dtype=torch.int64), z(2, dtype=torch.int64)
    pool, hdr = z(64, 96, dtype=torch.uint8), z(4, dtype=torch.int32)
    stream = P(torch.cuda.current_stream().cuda_stream)
    tail = (p(pool), p(hdr), stream) if pooled else (stream,)
    reset = lib.ka_shogi_env_reset_pool if pooled else lib.ka_shogi_env_reset
    step = lib.ka_shogi_env_step_pool if pooled else lib.ka_shogi_env_step
    rc = reset(p(state), p(keys), p(checks), n, MAX_PLY, 1, 1, p(obs[0]), p(mask[0]), p(bits[0]), p(players), 0, *tail)
    assert rc == 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cur, total = 0, 0.0
    for s in range(WARM + STEPS):
        if pooled and s == WARM:                      # positions of games in progress: playable by construction
            pool.copy_(state[:64, :96])
            hdr.copy_(torch.tensor([64, 0, 12345, 0], dtype=torch.int32))
        acts = torch.multinomial(mask[cur].float(), 1, generator=gen).squeeze(1)
        nxt = cur ^ 1
        a.record()
        rc = step(p(state), p(keys), p(checks), p(acts), n, MAX_PLY, 1, 1, p(mask[cur]), p(bits[cur]), p(err), p(obs[nxt]),
                  p(mask[nxt]), p(bits[nxt]), p(rewards), p(term), p(trunc), p(tobs), p(players), p(cap), p(reason), p(ply),
                  p(material), p(stats), *tail)
        b.record()
        torch.cuda.synchronize()
        assert rc == 0
        if s >= WARM:
            total += a.elapsed_time(b)
        cur = nxt
    assert int(err[1].item()) == 0
    return {"lib": label, "envs": n, "pool": pooled, "us_per_step": round(total / STEPS * 1e3, 2),
            "games_finished": int(stats[0].item())}


assert torch.cuda.is_available(), "needs a GPU"
for n in (128, 16384):
    for pooled in ((False, True) if has_pool else (False,)):
        print(json.dumps(run(n, pooled)), flush=True)
