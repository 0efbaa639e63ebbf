// Game log: the moves of the games played on the device, kept inside the ply (reference: the per-env move_history of
// shogi-gym's VecEnv, vec_env.rs:259, cleared on auto-reset, and the move lists of the showcase games).  The loops that play
// on the device (SelfPlayRollout, MatchArena) never hand a move to the host; this file remembers them on the device and
// hands whole finished games over at the owner's sync points.
//
// Per env: a move row of row_stride >= max_ply uint16 (an action index is < 11 259; the stride is even, rows are 4-byte aligned); kGlMeta int32
// {moves in the row, carried flag, games finished since begin, unused}; a start slot of 96 bytes = the first 96 bytes of the
// env's state row when the game began (board[81] hands[2][7] side).
// Log: game_cap records of a fixed stride, kGlHead int32 {env, plies, winner, termination reason, flags, black id, white id,
// the owner's ply counter, game number, 3 unused} + the 24 start words + the moves, two per word, low half first; the
// unused half of the last word is zero and the words behind it are not written.
// Cursor: {records committed, records dropped, plies logged, unused}; the host reads and zeroes it at its sync point.
//
// gamelog_step_kernel is ONE workgroup that walks the E envs in tiles of 256 (the second of the two forms the ordering
// allows: no workgroup waits for another because there is only one).  The rank of a finishing env is the running count of
// the tiles before plus a ballot scan in thread order, so records follow the committed ones in (ply, env) order whatever
// the geometry.  Per tile the four waves then copy the tile's committed games, a wave per game.  It is the only writer of
// the cursor: no atomics.
//
// The kernel has two forms of one body (the template parameter kEnv).  kEnv = false names the players of a game through a
// pair table indexed by env / envs_per_pair (the arena).  kEnv = true takes them per env (the league: side[e] the learner's
// colour, opp[e] its opponent's index, ids the learner's and the opponents' ids); header word 9 is then the learner's colour
// + 1, and the fourth meta word holds tag = ((opp << 1) | side) + 1 of the players who made the row's last move: a later move
// under another tag sets the carried flag, so a re-draw of side or opponent in the middle of a game needs no call of its
// own.  kEnv = false neither reads nor writes that word.
//
// gamelog_peek_kernel writes the games in progress as record-shaped rows into a caller's buffer, a wave per game as in the
// copy phase above; it reads the log's buffers and writes nothing but those rows.
#include "common.h"

namespace {

constexpr int kGlThreads = 256;
constexpr int kGlHead = 12, kGlStart = 24, kGlCursor = 4, kGlMeta = 4;
constexpr int kGlMaxEnvs = 16384;                              // one stall byte of LDS per group of envs
constexpr int kGlTruncOnly = 1, kGlCarried = 2;

struct GameLogArgs {
    int E, max_ply, game_cap, row_stride, rec_words;
    const uint8_t* state; int state_bytes;
    const long long* actions; const float* rewards; const uint8_t* terminated; const uint8_t* truncated;
    const uint8_t* pre_player; const uint8_t* reason; const int* nlegal; const int* live;
    const int* pairs; int pair_stride; int group; const int* ply_counter;
    const uint8_t* side; const int* opp; const int* ids; int K;      // kEnv only
    uint16_t* rows; int* meta; int* starts; int* records; int* cursor;
};

__global__ __launch_bounds__(kGlThreads) void gamelog_begin_kernel(int E, const uint8_t* state, int state_bytes, int* meta,
                                                                   int* starts) {
    const int i = blockIdx.x * kGlThreads + threadIdx.x;      // one thread per start word
    if (i >= E * kGlStart) return;
    const int e = i / kGlStart, w = i - e * kGlStart;
    starts[i] = reinterpret_cast<const int*>(state + (size_t)e * state_bytes)[w];
    if (w < kGlMeta) meta[e * kGlMeta + w] = 0;
}

// the ids of env e's players from its learner side and opponent index: an index outside [0, K) names nobody (-1) and reads
// ids[0] in its place
__device__ __forceinline__ void gamelog_env_players(const int* ids, int K, int s, int k, int* black, int* white) {
    const bool ok = (unsigned)k < (unsigned)K;
    const int other = ids[ok ? k + 1 : 0], me = ids[0];
    const int oid = ok ? other : -1;
    *black = s ? oid : me;
    *white = s ? me : oid;
}

template <bool kEnv>
__global__ __launch_bounds__(kGlThreads) void gamelog_step_kernel(GameLogArgs a) {
    __shared__ int wsum[kGlThreads / 64];
    __shared__ int s_env[kGlThreads];                          // the tile's committed games: env and record index
    __shared__ int s_rec[kGlThreads];
    __shared__ int s_n[kGlThreads];
    __shared__ uint8_t s_stall[kGlMaxEnvs];                    // per group: an env of it had no legal action
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, E = a.E;
    const int G = a.group, groups = (E + G - 1) / G;
    for (int g = tid; g < groups; g += kGlThreads) s_stall[g] = 0;
    __syncthreads();
    if (a.nlegal)
        for (int e = tid; e < E; e += kGlThreads)
            if (a.nlegal[e] == 0) s_stall[e / G] = 1;          // (every writer stores the same byte)
    __syncthreads();
    const int first = a.cursor[0];
    const int room = first < 0 ? 0 : max(0, a.game_cap - first);
    const int owner_ply = a.ply_counter ? *a.ply_counter : 0;
    int running = 0;
    for (int tile = 0; tile < E; tile += kGlThreads) {
        const int k = tile + tid;
        const bool have = k < E;
        const int e = have ? k : 0;                            // loads are not branched around: a lane without an env reads env 0
        int* m = a.meta + (size_t)e * kGlMeta;
        const int action = (int)a.actions[e];
        const int count = m[0];
        const bool tm = a.terminated[e] != 0, tr = a.truncated[e] != 0;
        const bool is_live = a.live ? a.live[e] >= 0 : true;
        const float r = a.rewards[e];
        const int pre = a.pre_player[e] & 1;
        const int why = a.reason[e];
        const int game = m[2];
        const bool done = have && (tm || tr);
        int carried = (m[1] | (is_live ? 0 : 1)) & 1;
        int s = 0, tag = 0, black = -1, white = -1;
        if constexpr (kEnv) {
            s = a.side[e] & 1;
            const int ko = a.opp[e], last = m[3];
            tag = (int)((((unsigned)ko << 1) | (unsigned)s) + 1u);
            if (count > 0 && last != tag) carried = 1;         // the players changed since the row's last move
            gamelog_env_players(a.ids, a.K, s, ko, &black, &white);
        }
        const int plies = min(count + 1, a.max_ply);
        if (have) {
            if ((unsigned)count < (unsigned)a.max_ply) a.rows[(size_t)e * a.row_stride + count] = (uint16_t)action;
            m[0] = done ? 0 : plies;
            m[1] = done ? 0 : carried;
            m[2] = game + (done ? 1 : 0);
            if constexpr (kEnv) m[3] = done ? 0 : tag;
        }
        const bool commit = done && is_live && !s_stall[e / G];
        int rank;
        const int tot = ka_tile_rank(commit, running, wsum, &rank);        // (its barriers also guard s_env / s_rec)
        const bool fits = commit && rank < room;
        if (fits) {
            const int slot = rank - running;                   // place among the tile's committed games
            s_env[slot] = e;
            s_rec[slot] = first + rank;
            s_n[slot] = plies;
            int* rec = a.records + (size_t)(first + rank) * a.rec_words;
            if constexpr (!kEnv) {
                if (a.pairs) {
                    const int* p = a.pairs + (size_t)(e / G) * a.pair_stride;
                    black = p[0]; white = p[1];
                }
            }
            rec[0] = e; rec[1] = plies;
            rec[2] = r > 0.f ? pre : (r < 0.f ? 1 - pre : 2);   // the mover's reward; a NaN is a draw
            rec[3] = why;
            rec[4] = ((tr && !tm) ? kGlTruncOnly : 0) | (carried ? kGlCarried : 0);
            rec[5] = black; rec[6] = white; rec[7] = owner_ply; rec[8] = game;
            rec[9] = kEnv ? s + 1 : 0; rec[10] = 0; rec[11] = 0;
        }
        const int kept = max(0, min(tot, room - running));     // the tile's games that fit: its first `kept` by rank
        running += tot;
        __syncthreads();
        for (int j = wave; j < kept; j += kGlThreads / 64) {   // a wave per game: start position, then the moves
            const int ge = s_env[j];
            int* rec = a.records + (size_t)s_rec[j] * a.rec_words;
            const int n = s_n[j];
            const int* start = a.starts + (size_t)ge * kGlStart;
            if (lane < kGlStart) rec[kGlHead + lane] = start[lane];
            const uint32_t* row = reinterpret_cast<const uint32_t*>(a.rows + (size_t)ge * a.row_stride);
            uint32_t* dst = reinterpret_cast<uint32_t*>(rec + kGlHead + kGlStart);
            const int words = (n + 1) >> 1;
            for (int i = lane; i < words; i += 64) {
                const uint32_t v = row[i];
                dst[i] = (2 * i + 1 < n) ? v : (v & 0xffffu);
            }
        }
        __syncthreads();                                       // the records hold the old start before it is reloaded
        if (done) {                                            // the env kernel has restarted the game in the state row
            const int* src = reinterpret_cast<const int*>(a.state + (size_t)e * a.state_bytes);
            int* start = a.starts + (size_t)e * kGlStart;
            for (int w = 0; w < kGlStart; ++w) start[w] = src[w];
        }
    }
    if (tid == 0) {
        a.cursor[0] = first + min(running, room);
        a.cursor[1] += max(0, running - room);
        a.cursor[2] += 1;
    }
}

// jobs: n rows of {slot, ...} as ka_arena_assign takes them; one workgroup per job
__global__ __launch_bounds__(kGlThreads) void gamelog_seat_kernel(const int* jobs, int slots, int E, int* meta) {
    const int s = jobs[blockIdx.x * 4];
    if (s < 0 || s >= slots) return;
    for (int k = threadIdx.x; k < E; k += kGlThreads) {
        int* m = meta + ((size_t)s * E + k) * kGlMeta;
        if (m[0] > 0) m[1] = 1;                                // the new pairing inherits a game in progress
    }
}

struct GamePeekArgs {
    const int* list; int n; int E, max_ply, row_stride, rec_words;
    const int* pairs; int pair_stride; int group;
    const uint8_t* side; const int* opp; const int* ids; int K;
    const int* ply_counter;
    const uint16_t* rows; const int* meta; const int* starts; int* out;
};

// a wave per game in progress; every branch on the game is uniform over its wave
__global__ __launch_bounds__(kGlThreads) void gamelog_peek_kernel(GamePeekArgs a) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (kGlThreads / 64) + (threadIdx.x >> 6);
    if (j >= a.n) return;
    int* rec = a.out + (size_t)j * a.rec_words;
    const int idx = a.list ? a.list[j] : j;
    const int owner_ply = a.ply_counter ? *a.ply_counter : 0;
    if ((unsigned)idx >= (unsigned)a.E) {                      // no such env: an empty row, no env buffer is read
        if (lane < kGlHead) rec[lane] = (lane == 0 || lane == 2 || lane == 5 || lane == 6) ? -1 : (lane == 7 ? owner_ply : 0);
        if (lane < kGlStart) rec[kGlHead + lane] = 0;
        return;
    }
    const int e = idx;
    const int* m = a.meta + (size_t)e * kGlMeta;
    const int n = max(0, min(m[0], a.max_ply));
    if (lane == 0) {
        int black = -1, white = -1, colour = 0;
        if (a.pairs) {
            const int* p = a.pairs + (size_t)(e / a.group) * a.pair_stride;
            black = p[0]; white = p[1];
        } else if (a.side) {
            const int s = a.side[e] & 1;
            gamelog_env_players(a.ids, a.K, s, a.opp[e], &black, &white);
            colour = s + 1;
        }
        rec[0] = e; rec[1] = n; rec[2] = -1; rec[3] = 0;
        rec[4] = (m[1] & 1) ? kGlCarried : 0;
        rec[5] = black; rec[6] = white; rec[7] = owner_ply; rec[8] = m[2];
        rec[9] = colour; rec[10] = 0; rec[11] = 0;
    }
    const int* start = a.starts + (size_t)e * kGlStart;
    if (lane < kGlStart) rec[kGlHead + lane] = start[lane];
    const uint32_t* row = reinterpret_cast<const uint32_t*>(a.rows + (size_t)e * a.row_stride);
    uint32_t* dst = reinterpret_cast<uint32_t*>(rec + kGlHead + kGlStart);
    const int words = (n + 1) >> 1;
    for (int i = lane; i < words; i += 64) {
        const uint32_t v = row[i];
        dst[i] = (2 * i + 1 < n) ? v : (v & 0xffffu);
    }
}

}  // namespace

extern "C" int ka_gamelog_words(int which, int max_ply) {
    const int row = max_ply >= 0 ? (max_ply + 1) / 2 : 0;
    return which == 0 ? kGlHead + kGlStart + row : which == 1 ? kGlCursor : which == 2 ? kGlMeta : which == 3 ? row
         : which == 4 ? kGlHead : which == 5 ? kGlStart : which == 6 ? kGlMaxEnvs : -1;
}

extern "C" int ka_gamelog_begin(const void* env_state, int state_bytes, int envs, int* meta, int* starts, void* stream) {
    KA_REQUIRE(env_state && meta && starts, "gamelog_begin: null tensor");
    KA_REQUIRE(envs > 0 && envs <= kGlMaxEnvs, "gamelog_begin: envs %d (1..%d)", envs, kGlMaxEnvs);
    KA_REQUIRE(state_bytes >= 4 * kGlStart && state_bytes % 4 == 0 && (uintptr_t)env_state % 4 == 0,
               "gamelog_begin: state rows of %d bytes (at least 96, 4-byte aligned)", state_bytes);
    hipLaunchKernelGGL(gamelog_begin_kernel, dim3((envs * kGlStart + kGlThreads - 1) / kGlThreads), dim3(kGlThreads), 0,
                       static_cast<hipStream_t>(stream), envs, static_cast<const uint8_t*>(env_state), state_bytes, meta, starts);
    return ka_check_launch("gamelog_begin");
}

namespace {

int gamelog_step_check(const char* who, const void* env_state, int state_bytes, int envs, int max_ply, const void* actions,
                       const void* rewards, const void* terminated, const void* truncated, const void* pre_player,
                       const void* term_reason, const void* rows, int row_stride, const void* meta, const void* starts,
                       const void* records, int game_cap, const void* cursor) {
    KA_REQUIRE(env_state && actions && rewards && terminated && truncated && pre_player && term_reason && rows && meta &&
               starts && records && cursor, "%s: null tensor", who);
    KA_REQUIRE(envs > 0 && envs <= kGlMaxEnvs, "%s: envs %d (1..%d)", who, envs, kGlMaxEnvs);
    KA_REQUIRE(max_ply >= 1 && max_ply <= 65535, "%s: max_ply %d (1..65535)", who, max_ply);
    KA_REQUIRE(state_bytes >= 4 * kGlStart && state_bytes % 4 == 0 && (uintptr_t)env_state % 4 == 0,
               "%s: state rows of %d bytes (at least 96, 4-byte aligned)", who, state_bytes);
    KA_REQUIRE((uintptr_t)rows % 4 == 0 && row_stride % 2 == 0 && row_stride >= max_ply,
               "%s: move rows of %d uint16 (even, at least max_ply %d, 4-byte aligned)", who, row_stride, max_ply);
    const int rec_words = kGlHead + kGlStart + (max_ply + 1) / 2;
    KA_REQUIRE(game_cap >= 0 && (long long)game_cap * rec_words < (1ll << 31), "%s: game_cap %d x %d words", who, game_cap,
               rec_words);
    return 0;
}

}  // namespace

extern "C" int ka_gamelog_step(const void* env_state, int state_bytes, int envs, int max_ply, const long long* actions,
                               const float* rewards, const void* terminated, const void* truncated, const void* pre_player,
                               const void* term_reason, const int* nlegal, const int* live, const int* pairs, int pair_stride,
                               int envs_per_pair, const int* ply_counter, void* rows, int row_stride, int* meta, int* starts,
                               int* records, int game_cap, int* cursor, void* stream) {
    if (int rc = gamelog_step_check("gamelog_step", env_state, state_bytes, envs, max_ply, actions, rewards, terminated,
                                    truncated, pre_player, term_reason, rows, row_stride, meta, starts, records, game_cap, cursor))
        return rc;
    KA_REQUIRE(!pairs || (pair_stride >= 2 && envs_per_pair > 0), "gamelog_step: pair_stride %d (>= 2), envs_per_pair %d (> 0)",
               pair_stride, envs_per_pair);
    GameLogArgs a{envs, max_ply, game_cap, row_stride, kGlHead + kGlStart + (max_ply + 1) / 2,
                  static_cast<const uint8_t*>(env_state), state_bytes, actions,
                  rewards, static_cast<const uint8_t*>(terminated), static_cast<const uint8_t*>(truncated),
                  static_cast<const uint8_t*>(pre_player), static_cast<const uint8_t*>(term_reason), nlegal, live, pairs,
                  pair_stride, pairs ? envs_per_pair : 1, ply_counter, nullptr, nullptr, nullptr, 0,
                  static_cast<uint16_t*>(rows), meta, starts, records, cursor};
    hipLaunchKernelGGL(gamelog_step_kernel<false>, dim3(1), dim3(kGlThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("gamelog_step");
}

extern "C" int ka_gamelog_step_env(const void* env_state, int state_bytes, int envs, int max_ply, const long long* actions,
                                   const float* rewards, const void* terminated, const void* truncated,
                                   const void* pre_player, const void* term_reason, const int* nlegal, const int* live,
                                   const void* side, const int* opp, const int* ids, int opponents, const int* ply_counter,
                                   void* rows, int row_stride, int* meta, int* starts, int* records, int game_cap, int* cursor,
                                   void* stream) {
    if (int rc = gamelog_step_check("gamelog_step_env", env_state, state_bytes, envs, max_ply, actions, rewards, terminated,
                                    truncated, pre_player, term_reason, rows, row_stride, meta, starts, records, game_cap, cursor))
        return rc;
    KA_REQUIRE(side && opp && ids, "gamelog_step_env: null side / opp / ids");
    KA_REQUIRE(opponents >= 0, "gamelog_step_env: opponents %d (>= 0)", opponents);
    GameLogArgs a{envs, max_ply, game_cap, row_stride, kGlHead + kGlStart + (max_ply + 1) / 2,
                  static_cast<const uint8_t*>(env_state), state_bytes, actions,
                  rewards, static_cast<const uint8_t*>(terminated), static_cast<const uint8_t*>(truncated),
                  static_cast<const uint8_t*>(pre_player), static_cast<const uint8_t*>(term_reason), nlegal, live, nullptr,
                  0, 1, ply_counter, static_cast<const uint8_t*>(side), opp, ids, opponents,
                  static_cast<uint16_t*>(rows), meta, starts, records, cursor};
    hipLaunchKernelGGL(gamelog_step_kernel<true>, dim3(1), dim3(kGlThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("gamelog_step_env");
}

extern "C" int ka_gamelog_peek(const int* envs_list, int n, int envs, int max_ply, const int* pairs, int pair_stride,
                               int envs_per_pair, const void* side, const int* opp, const int* ids, int opponents,
                               const int* ply_counter, const void* rows, int row_stride, const int* meta, const int* starts,
                               int* out, void* stream) {
    KA_REQUIRE(rows && meta && starts && out, "gamelog_peek: null tensor");
    KA_REQUIRE(envs > 0 && envs <= kGlMaxEnvs, "gamelog_peek: envs %d (1..%d)", envs, kGlMaxEnvs);
    KA_REQUIRE(max_ply >= 1 && max_ply <= 65535, "gamelog_peek: max_ply %d (1..65535)", max_ply);
    KA_REQUIRE((uintptr_t)rows % 4 == 0 && row_stride % 2 == 0 && row_stride >= max_ply,
               "gamelog_peek: move rows of %d uint16 (even, at least max_ply %d, 4-byte aligned)", row_stride, max_ply);
    const int rec_words = kGlHead + kGlStart + (max_ply + 1) / 2;
    KA_REQUIRE(n > 0 && (long long)n * rec_words < (1ll << 31), "gamelog_peek: %d rows x %d words", n, rec_words);
    KA_REQUIRE(envs_list || n <= envs, "gamelog_peek: %d rows of %d envs without a list", n, envs);
    KA_REQUIRE(!(pairs && side), "gamelog_peek: players from pairs or from side / opp / ids, not both");
    KA_REQUIRE(!pairs || (pair_stride >= 2 && envs_per_pair > 0), "gamelog_peek: pair_stride %d (>= 2), envs_per_pair %d (> 0)",
               pair_stride, envs_per_pair);
    KA_REQUIRE(!side || (opp && ids && opponents >= 0), "gamelog_peek: side needs opp, ids and opponents %d (>= 0)", opponents);
    GamePeekArgs a{envs_list, n, envs, max_ply, row_stride, rec_words, pairs, pair_stride, pairs ? envs_per_pair : 1,
                   static_cast<const uint8_t*>(side), opp, ids, opponents, ply_counter, static_cast<const uint16_t*>(rows),
                   meta, starts, out};
    const int per = kGlThreads / 64;
    hipLaunchKernelGGL(gamelog_peek_kernel, dim3((n + per - 1) / per), dim3(kGlThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("gamelog_peek");
}

extern "C" int ka_gamelog_seat(const int* jobs, int njobs, int slots, int envs_per_slot, int* meta, void* stream) {
    KA_REQUIRE(jobs && meta, "gamelog_seat: null tensor");
    KA_REQUIRE(njobs > 0 && slots > 0 && envs_per_slot > 0 && (long long)slots * envs_per_slot <= kGlMaxEnvs,
               "gamelog_seat: njobs %d, slots %d, envs_per_slot %d", njobs, slots, envs_per_slot);
    hipLaunchKernelGGL(gamelog_seat_kernel, dim3(njobs), dim3(kGlThreads), 0, static_cast<hipStream_t>(stream), jobs, slots,
                       envs_per_slot, meta);
    return ka_check_launch("gamelog_seat");
}
