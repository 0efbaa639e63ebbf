// League rollout: the learner-vs-cohort bookkeeping of one rollout step on the device (reference:
// keisei/training/katago_loop.py:1219-1437, the opponent branch of KataGoTrainingLoop.run, and :1537-1563, the flush at
// the end of an epoch).  One ply is: grouped forward on model_of -> ka_policy_sample_play -> ka_shogi_env_step ->
// ka_league_step; the host looks at the state once per chunk of plies.
//
// ka_league_step is two launches on one stream:
//   league_plan_kernel  ONE workgroup.  It walks the E envs in tiles of 256 and does everything that is a word per env or
//                       a counter: learner-frame rewards and tallies, the settle / open / immediate-settle decisions, the
//                       store row of every settled transition (ballot ranks, env order), the scalar columns of those
//                       rows, the pending slots' scalars, per-opponent results, the re-draws and the next model_of.  It
//                       is the only reader and writer of every cursor, so no workgroup reads a word another one writes.
//   league_copy_kernel  one workgroup per env: the big rows the plan asks for (pending observation + mask -> store row,
//                       this ply's observation + mask -> store row or pending slot, terminal observation -> truncation
//                       slot).
// No atomics anywhere: counters are block sums, ranks are ballot scans in thread order.
//
// State: ka_league_state_words(K) int32, read by the host in one copy.  The words shared with the self-play step are
// tabulated in rollout_rows.h (the tallies are in the learner's frame); the league's own:
//   2     plies stepped since the last reset
//   4     non-empty blocks written (the reference's add() calls)
//   10-11 draw seed (int64), fixed between resets
//   25    a pending slot was opened while still taken
//   26    bit 0: a learner row had no legal action, bit 1: an opponent row (the envs are latched in `stall`)
//   27-31 unused
//   32..  K x {wins, losses, draws} per opponent, learner frame
//
// Draws (documented in include/keisei_amd.h): mix(x) is the splitmix64 finaliser ka_policy_sample uses,
//   h(salt, env, n) = mix(draw_seed ^ mix((env << 32 | n) + salt)),  n = games finished in that env since the reset
//   opponent = first k with (h(0x6F70706F, env, n) >> 33) < cum[k]   (cum: K uint32 thresholds on a 31-bit scale, the last 2^31)
//   side     = h(0x73696465, env, n) >> 63
// A function of (seed, env, n) alone: the same whatever sync_every, graph capture or launch geometry.
#include "rollout_rows.h"

namespace {

constexpr int kLgThreads = 256;
constexpr int kLgHdr = 32, kLgPlan = 6;
enum { kPly = 2, kBlocks = 4, kDrawSeed = 10, kConflict = 25, kStall = 26 };      // the league's own state words
// pending scalars: kPendCols columns of E words {action, log-prob, value, reward, score target, valid}
enum { kPAction = 0, kPLogp = 1, kPValue = 2, kPReward = 3, kPScore = 4, kPValid = 5, kPendCols = 6 };
constexpr unsigned long long kSaltOpp = 0x6F70706Full, kSaltSide = 0x73696465ull;

__device__ __forceinline__ unsigned long long league_draw(unsigned long long seed, unsigned long long salt, int env, int n) {
    return ka_mix64(seed ^ ka_mix64((((unsigned long long)(unsigned)env << 32) | (unsigned)n) + salt));
}

struct LeagueArgs {
    int* state; int E, K, flush;
    // the ply before the env step
    const float* obs; const uint32_t* bits; const long long* actions; const float* logp; const float* vlogits;
    const float* score_lead; float alpha; const int* nlegal; const uint8_t* pre_player;
    // the env step's result
    const float* rewards; const uint8_t* terminated; const uint8_t* truncated; const uint8_t* players; const int* material;
    float score_norm; const float* term_obs; const long long* refusal;
    // league state per env
    uint8_t* side; int* opp; int* games; const uint32_t* cum; int color_rand; int* model_of; uint8_t* stall; float* values;
    // pending slots
    float* p_obs; uint32_t* p_bits; int* p_scal;
    // truncation slots: E observation rows and E x {env, store row, player to move | learner side << 1}
    float* t_obs; int* t_list;
    const long long* desc;                     // 12 column base pointers, base row, reserved rows behind it
    int* plan;                                 // E x {row of the earlier block, row of the immediate block, truncation slot of
                                               //      either, keep-pending flag, unused}: store rows are absolute, -1 = none
    int obs_elems, words;
};

__global__ __launch_bounds__(kLgThreads) void league_plan_kernel(LeagueArgs a) {
    extern __shared__ short s_code[];                          // E: opponent * 3 + outcome of a terminated game, -1 = none
    __shared__ int red[kLgThreads / 64];
    __shared__ int wsum[kLgThreads / 64];
    const int tid = threadIdx.x, E = a.E;
    const bool step = !a.flush;
    const Columns c = load_columns(a.desc);
    int* st = a.state;
    const int first = st[kRows], tfirst = st[kTrunc];
    const long long room = c.cap > first ? c.cap - first : 0;
    const unsigned long long dseed = *reinterpret_cast<const unsigned long long*>(st + kDrawSeed);
    int* P = a.p_scal;

    // the reference's flags of env k this ply
    auto facts = [&](int k, bool& lm, bool& done, bool& tm, bool& settle, bool& open, bool& conflict) {
        const bool valid = P[kPValid * E + k] != 0;
        if (!step) {                                           // :1537-1563: everything still pending, done = terminated = 0
            lm = done = tm = open = conflict = false;
            settle = valid;
            return;
        }
        const int sd = a.side[k];
        lm = (a.pre_player[k] & 1) == sd;
        const bool ln = (a.players[k] & 1) == sd;
        tm = a.terminated[k] != 0;
        done = tm || a.truncated[k] != 0;
        settle = valid && (done || ln);                        // :1296
        conflict = lm && valid && !settle;                     // create() on a slot still taken (:187-191)
        open = lm && !conflict;
    };

    // pass 1: sizes of the earlier block and of its truncation records (the immediate block sits behind them)
    int n1 = 0, nt1 = 0;
    for (int k = tid; k < E; k += kLgThreads) {
        bool lm, done, tm, settle, open, conflict;
        facts(k, lm, done, tm, settle, open, conflict);
        n1 += settle;
        nt1 += settle && done && !tm;
    }
    n1 = ka_block_sum<kLgThreads>(n1, red);
    nt1 = ka_block_sum<kLgThreads>(nt1, red);

    int run1 = 0, run2 = 0, runt1 = 0, runt2 = 0;
    int conflicts = 0, stall = 0, dropped = 0, tdropped = 0;
    Tallies tl{};
    RowGuards g{0, 0, 0, 0};
    for (int base = 0; base < E; base += kLgThreads) {
        const int k = base + tid;
        const bool have = k < E;
        bool lm = false, done = false, tm = false, settle = false, open = false, conflict = false;
        if (have) facts(k, lm, done, tm, settle, open, conflict);
        const bool imm = open && done;                         // :1344
        const bool trunc_only = done && !tm;
        int r1, r2, t1, t2;
        run1 += ka_tile_rank(settle, run1, wsum, &r1);
        run2 += ka_tile_rank(imm, run2, wsum, &r2);
        runt1 += ka_tile_rank(settle && trunc_only, runt1, wsum, &t1);
        runt2 += ka_tile_rank(imm && trunc_only, runt2, wsum, &t2);
        if (!have) continue;
        const float r = step ? a.rewards[k] : 0.f;
        const float lr = lm ? r : -r;                           // to_learner_perspective (:111-122)
        const int pre = step ? (a.pre_player[k] & 1) : 0;
        int* plan = a.plan + (size_t)k * kLgPlan;
        long long row1 = -1, row2 = -1;
        int ts1 = -1, ts2 = -1;
        // 1. tallies (:1219-1248)
        if (step) {
            tally_add(tl, tm, trunc_only, lr, r, pre);
            conflicts += conflict;
            if (a.nlegal[k] == 0) { const int bit = lm ? 1 : 2; stall |= bit; a.stall[k] |= bit; }
        }
        // 2. accumulate and settle earlier transitions (:1290-1316)
        const bool valid = P[kPValid * E + k] != 0;
        float prew = __int_as_float(P[kPReward * E + k]);
        if (valid && step) prew += lr;
        if (settle) {
            if (r1 < room) {
                row1 = c.base + first + r1;
                write_row(c, row1, k, P[kPAction * E + k], __int_as_float(P[kPLogp * E + k]), __int_as_float(P[kPValue * E + k]),
                          prew, done, tm, __int_as_float(P[kPScore * E + k]), step, &g);
            } else {
                dropped += 1;
            }
            prew = 0.f;
        }
        // 3. open a slot where the learner just moved (:1319-1341); 4. settle it at once if that ended the game (:1343-1365)
        float value = 0.f;
        if (step && lm)                                         // katago_ppo.py:536-541 / value_adapter.py:56-65, as ka_policy_sample
            value = ka_blended_value(a.vlogits + k * 3, a.score_lead ? a.score_lead + k : nullptr, a.alpha);
        if (step) a.values[k] = value;
        bool keep = false;
        if (open) {
            const float score = (float)a.material[k] / a.score_norm;
            if (imm) {
                const long long i2 = (long long)n1 + r2;
                if (i2 < room) {
                    row2 = c.base + first + i2;
                    write_row(c, row2, k, a.actions[k], a.logp[k], value, lr, done, tm, score, true, &g);
                } else {
                    dropped += 1;
                }
            } else {
                keep = true;
                P[kPAction * E + k] = (int)a.actions[k];
                P[kPLogp * E + k] = __float_as_int(a.logp[k]);
                P[kPValue * E + k] = __float_as_int(value);
                P[kPScore * E + k] = __float_as_int(score);
                prew = lr;
            }
        }
        P[kPReward * E + k] = __float_as_int(prew);
        P[kPValid * E + k] = (valid && !settle) || keep;
        // truncation bootstrap override, deferred (:1250-1283): the terminal observation goes to a slot, the host fills the row
        if (settle && trunc_only && row1 >= 0) {
            const int slot = tfirst + t1;
            if (slot < E) ts1 = slot; else tdropped += 1;
        }
        if (imm && trunc_only && row2 >= 0) {
            const int slot = tfirst + nt1 + t2;
            if (slot < E) ts2 = slot; else tdropped += 1;
        }
        if (ts1 >= 0 || ts2 >= 0) {
            const int who = (1 - pre) | (a.side[k] << 1);
            if (ts1 >= 0) { int* t = a.t_list + ts1 * 3; t[0] = k; t[1] = (int)row1; t[2] = who; }
            if (ts2 >= 0) { int* t = a.t_list + ts2 * 3; t[0] = k; t[1] = (int)row2; t[2] = who; }
        }
        plan[0] = (int)row1; plan[1] = (int)row2; plan[2] = ts1; plan[3] = ts2; plan[4] = keep; plan[5] = 0;
        if (!step) continue;
        // 5. per-opponent results of terminated games, by the opponent that played the game (:1384-1407)
        int o = a.opp[k];
        s_code[k] = (tm && o >= 0 && o < a.K) ? (short)(o * 3 + (lr > 0.f ? 0 : (lr < 0.f ? 1 : 2))) : (short)-1;
        // 6. / 7. a finished game: next opponent, next side (:1409-1437)
        int sd = a.side[k];
        if (done) {
            const int n = a.games[k] + 1;
            a.games[k] = n;
            const unsigned u = (unsigned)(league_draw(dseed, kSaltOpp, k, n) >> 33);
            o = a.K - 1;
            for (int j = 0; j < a.K; ++j) if (u < a.cum[j]) { o = j; break; }
            a.opp[k] = o;
            if (a.color_rand) {
                sd = (int)(league_draw(dseed, kSaltSide, k, n) >> 63);
                a.side[k] = (uint8_t)sd;
            }
        }
        // 8. seat the next ply: slot 0 is the learner, slot o + 1 opponent o
        a.model_of[k] = (a.players[k] & 1) == sd ? 0 : o + 1;
    }
    constexpr int T = kLgThreads;
    commit_tallies_and_guards<T>(tl, g, st, red);              // (a flush tallies nothing: it adds zeros)
    conflicts = ka_block_sum<T>(conflicts, red); stall = ka_block_max<T>(stall & 1, red) | (ka_block_max<T>(stall & 2, red));
    dropped = ka_block_sum<T>(dropped, red); tdropped = ka_block_sum<T>(tdropped, red);
    if (tid == 0) {
        const int offered = run1 + run2;
        st[kRows] = first + (int)min((long long)offered, room);
        st[kBlocks] += (run1 > 0) + (run2 > 0);
        st[kDropped] += dropped;
        st[kTrunc] = min(E, tfirst + runt1 + runt2);
        st[kTruncDropped] += tdropped;
        if (step) {
            ply_tail(st, kRefusal, a.refusal);
            st[kPly] += 1;
            st[kConflict] |= conflicts > 0; st[kStall] |= stall;
        }
    }
    if (!step) return;
    // per-opponent counters: wave w counts codes w, w + 4, ... by ballots over the envs
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int code = wave; code < a.K * 3; code += kLgThreads / 64) {
        int n = 0;
        for (int base = 0; base < E; base += 64) {
            const int k = base + lane;
            n += __popcll(__ballot(k < E && s_code[k] == code));
        }
        if (lane == 0 && n) st[kLgHdr + code] += n;
    }
}

__global__ __launch_bounds__(kLgThreads) void league_copy_kernel(LeagueArgs a) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const int* plan = a.plan + (size_t)e * kLgPlan;
    const int row1 = plan[0], row2 = plan[1], ts1 = plan[2], ts2 = plan[3], keep = plan[4];
    if (row1 < 0 && row2 < 0 && !keep) return;                  // (a truncation slot always comes with a row)
    const Columns c = load_columns(a.desc);
    const size_t n = a.obs_elems;
    // the pending slot leaves before this ply's move takes it
    if (row1 >= 0) copy_transition<kLgThreads>(c.obs, c.bits, row1, a.p_obs, a.p_bits, e, a.obs_elems, a.words);
    if (ts1 >= 0) ka_copy_row<kLgThreads>(a.t_obs + ts1 * n, a.term_obs + e * n, a.obs_elems, tid);
    if (ts2 >= 0) ka_copy_row<kLgThreads>(a.t_obs + ts2 * n, a.term_obs + e * n, a.obs_elems, tid);
    if (row2 >= 0) copy_transition<kLgThreads>(c.obs, c.bits, row2, a.obs, a.bits, e, a.obs_elems, a.words);
    if (keep) {
        __syncthreads();                                        // row1's reads of the slot are done
        copy_transition<kLgThreads>(a.p_obs, a.p_bits, e, a.obs, a.bits, e, a.obs_elems, a.words);
    }
}

}  // namespace

extern "C" int ka_league_state_words(int opponents) { return opponents < 0 ? -1 : kLgHdr + 3 * opponents; }
// which: 0 = int32 words of one env's plan, 1 = int64 words of the store descriptor, 2 = int32 words of one env's pending
// scalars, 3 = int32 words of one truncation record, 4 = the largest number of envs
extern "C" int ka_league_layout(int which) {
    return which == 0 ? kLgPlan : which == 1 ? kRolloutDesc : which == 2 ? kPendCols : which == 3 ? 3 : which == 4 ? kRolloutMaxEnvs : -1;
}

extern "C" int ka_league_step(int* state, int envs, int opponents, int flush, const float* obs, const void* mask_bits,
                              const long long* actions, const float* logp, const float* vlogits, const float* score_lead,
                              float alpha, const int* nlegal, const void* pre_player, const float* rewards,
                              const void* terminated, const void* truncated, const void* players, const int* material,
                              float score_norm, const float* term_obs, const long long* refusal, void* side, int* opp,
                              int* games, const void* cum, int color_rand, int* model_of, void* stall, float* values,
                              float* p_obs, void* p_bits, int* p_scal, float* t_obs, int* t_list, const long long* desc,
                              int* plan, int obs_elems, int mask_words, void* stream) {
    KA_REQUIRE(state && p_obs && p_bits && p_scal && desc && plan, "league_step: null state, pending slots, descriptor or plan");
    KA_REQUIRE_ROLLOUT_STEP("league_step", envs, obs_elems, mask_words, flush ? 1.f : score_norm);     // a flush reads no score_norm
    if (!flush) {
        KA_REQUIRE(obs && mask_bits && actions && logp && vlogits && nlegal && pre_player && rewards && terminated &&
                   truncated && players && material && term_obs && side && opp && games && cum && model_of && stall &&
                   values && t_obs && t_list, "league_step: null tensor");
        KA_REQUIRE(opponents > 0 && opponents <= 10000, "league_step: opponents %d (1..10000)", opponents);
    }
    LeagueArgs a{state, envs, opponents, flush ? 1 : 0, obs, static_cast<const uint32_t*>(mask_bits), actions, logp, vlogits,
                 score_lead, alpha, nlegal, static_cast<const uint8_t*>(pre_player), rewards,
                 static_cast<const uint8_t*>(terminated), static_cast<const uint8_t*>(truncated),
                 static_cast<const uint8_t*>(players), material, score_norm, term_obs, refusal, static_cast<uint8_t*>(side),
                 opp, games, static_cast<const uint32_t*>(cum), color_rand, model_of, static_cast<uint8_t*>(stall), values,
                 p_obs, static_cast<uint32_t*>(p_bits), p_scal, t_obs, t_list, desc, plan, obs_elems, mask_words};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(league_plan_kernel, dim3(1), dim3(kLgThreads), envs * sizeof(short), st, a);
    hipLaunchKernelGGL(league_copy_kernel, dim3(envs), dim3(kLgThreads), 0, st, a);
    return ka_check_launch("league_step");
}
