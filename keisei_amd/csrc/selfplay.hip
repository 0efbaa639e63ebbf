// Self-play rollout: the bookkeeping of one rollout step of the no-opponent branch on the device (reference:
// keisei/training/katago_loop.py:1438-1527; every env is the learner, every ply gives one transition per env).  One ply is:
// grouped forward (one model) -> ka_policy_sample_play -> ka_shogi_env_step -> ka_selfplay_step; the host looks at the
// state once per chunk of plies.
//
// ka_selfplay_step is two launches on one stream:
//   selfplay_plan_kernel  ONE workgroup.  It walks the E envs in tiles of 256 and does everything that is a word per env or
//                         a counter: the tallies, the scalar columns of the env's row, the input guards, the truncation
//                         slots (ballot ranks, env order), the state.  It is the only reader and writer of every counter.
//   selfplay_copy_kernel  one workgroup per env: the pre-step observation and packed mask into the env's row, the terminal
//                         observation of a truncated game into its slot.
// Env e at ply p of the epoch owns store row base + p * E + e (the dense (T, N) layout, no env_ids), so no row needs a
// rank; the truncation slots do, and get it from ballot scans in thread order.  No atomics anywhere.
//
// State: ka_selfplay_state_words() int32, read by the host in one copy.
//   0-1   seed (int64) ka_policy_sample_play reads this ply; advanced by a Weyl step per ply
//   2     ply of the epoch: the p of the row rule.  The kernel advances it, the host zeroes it when a collect begins
//   3     rows written behind the descriptor's base row
//   4     plies stepped since the last reset (the host never clears it between resets)
//   5     rows that did not fit the reserved capacity
//   6-7   the sampler's flags [NaN logits, a row without a legal action]
//   8-9   copy of the VecEnv refusal latch (int64)
//   10-11 unused
//   12    truncation slots used since the host last cleared it
//   13    truncations that found no slot
//   14-20 wins, losses, draws (the mover's frame), black wins, white wins, terminated, truncated-only
//   21-24 the rollout store's input guards over the rows written: terminated without done, value category outside
//         {-1, 0, 1, 2}, NaN score target, bits of max |score target|  (ka_rollout_append's four flags)
//   25    an env had no legal action (the envs are latched in `stall`)
//   26-31 unused
#include "common.h"

namespace {

constexpr int kSpThreads = 256;
constexpr int kSpWords = 32, kSpPlan = 2, kSpDesc = 14, kSpTrunc = 2;
constexpr int kSpMaxEnvs = 4096;
enum { kSeed = 0, kPly = 2, kRows = 3, kPlies = 4, kDropped = 5, kSamp = 6, kRefusal = 8, kTrunc = 12, kTruncDropped = 13,
       kWins = 14, kLosses = 15, kDraws = 16, kBlack = 17, kWhite = 18, kTerminated = 19, kTruncated = 20, kGuards = 21,
       kStall = 25 };

struct SelfPlayArgs {
    int* state; int E;
    // the ply before the env step
    const float* obs; const uint32_t* bits; const long long* actions; const float* logp; const float* vlogits;
    const float* score_lead; float alpha; const int* nlegal; const uint8_t* pre_player;
    // the env step's result
    const float* rewards; const uint8_t* terminated; const uint8_t* truncated; const int* material; float score_norm;
    const float* term_obs; const long long* refusal;
    uint8_t* stall; float* values;
    float* t_obs; int* t_list;                 // truncation slots: E observation rows and E x {env, store row}
    const long long* desc;                     // 12 column base pointers (env_ids unused), base row, reserved rows behind it
    int* plan;                                 // E x {store row (absolute, -1 = none), truncation slot (-1 = none)}
    int obs_elems, words;
};

__global__ __launch_bounds__(kSpThreads) void selfplay_plan_kernel(SelfPlayArgs a) {
    __shared__ int red[kSpThreads / 64];
    __shared__ int wsum[kSpThreads / 64];
    const int tid = threadIdx.x, E = a.E;
    int* st = a.state;
    const long long* d = a.desc;
    long long* c_actions = reinterpret_cast<long long*>(d[2]);
    float* c_logp = reinterpret_cast<float*>(d[3]);
    float* c_values = reinterpret_cast<float*>(d[4]);
    float* c_rewards = reinterpret_cast<float*>(d[5]);
    uint8_t* c_dones = reinterpret_cast<uint8_t*>(d[6]);
    uint8_t* c_term = reinterpret_cast<uint8_t*>(d[7]);
    long long* c_cats = reinterpret_cast<long long*>(d[8]);
    float* c_score = reinterpret_cast<float*>(d[9]);
    float* c_override = reinterpret_cast<float*>(d[11]);
    const long long base = d[12], cap = d[13];
    const int ply = st[kPly], tfirst = st[kTrunc];
    const long long first = (long long)ply * E;               // this ply's first row behind the base row

    int runt = 0;
    int wins = 0, losses = 0, draws = 0, black = 0, white = 0, nterm = 0, ntrunc = 0, stall = 0, written = 0;
    int dropped = 0, tdropped = 0;
    int g_term = 0, g_cat = 0, g_nan = 0, g_peak = 0;
    for (int tile = 0; tile < E; tile += kSpThreads) {
        const int k = tile + tid;
        const bool have = k < E;
        const bool tm = have && a.terminated[k] != 0;
        const bool done = have && (tm || a.truncated[k] != 0);  // :1458
        const bool trunc_only = done && !tm;                    // :1502
        const bool fits = have && first + k < cap;
        int t;
        runt += ka_tile_rank(trunc_only && fits, runt, wsum, &t);
        if (!have) continue;
        const float r = a.rewards[k];                           // the mover's frame: no flip in this branch
        const int pre = a.pre_player[k] & 1;
        // tallies (:1460-1485)
        nterm += tm; ntrunc += trunc_only;
        if (tm) {
            wins += r > 0.f; losses += r < 0.f; draws += r == 0.f;
            black += (r > 0.f && pre == 0) || (r < 0.f && pre == 1);
            white += (r > 0.f && pre == 1) || (r < 0.f && pre == 0);
        }
        if (a.nlegal[k] == 0) { stall = 1; a.stall[k] = 1; }
        const float value = ka_blended_value(a.vlogits + k * 3, a.score_lead ? a.score_lead + k : nullptr, a.alpha);
        a.values[k] = value;                                    // :1446, latest_values
        int* plan = a.plan + (size_t)k * kSpPlan;
        if (!fits) {
            dropped += 1;
            plan[0] = -1; plan[1] = -1;
            continue;
        }
        // the row's scalar columns (:1487-1527; label: _compute_value_cats, :75-92)
        const long long row = base + first + k;
        const long long cat = !tm ? -1 : (r > 0.f ? 0 : (r == 0.f ? 1 : (r < 0.f ? 2 : 3)));
        const float score = (float)a.material[k] / a.score_norm;
        c_actions[row] = a.actions[k]; c_logp[row] = a.logp[k]; c_values[row] = value; c_rewards[row] = r;
        c_dones[row] = done; c_term[row] = tm; c_cats[row] = cat; c_score[row] = score;
        c_override[row] = __uint_as_float(0x7fc00000u);         // NaN: the host fills the truncated rows at the sync point
        written += 1;
        g_term |= tm && !done;
        g_cat |= cat < -1 || cat > 2;
        if (score != score) g_nan = 1;
        else g_peak = max(g_peak, __float_as_int(fabsf(score)));
        // truncation bootstrap override, deferred (:1496-1521): the terminal observation goes to a slot
        int ts = -1;
        if (trunc_only) {
            const int slot = tfirst + t;
            if (slot < E) { ts = slot; a.t_list[slot * kSpTrunc] = k; a.t_list[slot * kSpTrunc + 1] = (int)row; }
            else tdropped += 1;
        }
        plan[0] = (int)row; plan[1] = ts;
    }
    constexpr int T = kSpThreads;
    wins = ka_block_sum<T>(wins, red); losses = ka_block_sum<T>(losses, red); draws = ka_block_sum<T>(draws, red);
    black = ka_block_sum<T>(black, red); white = ka_block_sum<T>(white, red);
    nterm = ka_block_sum<T>(nterm, red); ntrunc = ka_block_sum<T>(ntrunc, red);
    written = ka_block_sum<T>(written, red); dropped = ka_block_sum<T>(dropped, red); tdropped = ka_block_sum<T>(tdropped, red);
    stall = ka_block_max<T>(stall, red);
    g_term = ka_block_max<T>(g_term, red); g_cat = ka_block_max<T>(g_cat, red); g_nan = ka_block_max<T>(g_nan, red);
    g_peak = ka_block_max<T>(g_peak, red);
    if (tid == 0) {
        auto* seed = reinterpret_cast<unsigned long long*>(st);
        *seed += kKaWeyl;                                       // next ply's sampler seed, as the arena's referee steps it
        st[kPly] = ply + 1;
        st[kPlies] += 1;
        st[kRows] += written;
        st[kDropped] += dropped;
        st[kTrunc] = min(E, tfirst + runt);
        st[kTruncDropped] += tdropped;
        if (a.refusal) *reinterpret_cast<long long*>(st + kRefusal) = *a.refusal;
        st[kWins] += wins; st[kLosses] += losses; st[kDraws] += draws; st[kBlack] += black; st[kWhite] += white;
        st[kTerminated] += nterm; st[kTruncated] += ntrunc;
        st[kGuards + 0] |= g_term; st[kGuards + 1] |= g_cat; st[kGuards + 2] |= g_nan;
        st[kGuards + 3] = max(st[kGuards + 3], g_peak);
        st[kStall] |= stall;
    }
}

__global__ __launch_bounds__(kSpThreads) void selfplay_copy_kernel(SelfPlayArgs a) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const long long row = a.plan[(size_t)e * kSpPlan];
    const int ts = a.plan[(size_t)e * kSpPlan + 1];
    if (row < 0) return;                                        // (a truncation slot always comes with a row)
    const size_t n = a.obs_elems, w = a.words;
    float* c_obs = reinterpret_cast<float*>(a.desc[0]);
    uint32_t* c_bits = reinterpret_cast<uint32_t*>(a.desc[1]);
    ka_copy_row<kSpThreads>(c_obs + row * n, a.obs + e * n, a.obs_elems, tid);
    for (int i = tid; i < a.words; i += kSpThreads) c_bits[row * w + i] = a.bits[e * w + i];
    if (ts >= 0) ka_copy_row<kSpThreads>(a.t_obs + ts * n, a.term_obs + e * n, a.obs_elems, tid);
}

}  // namespace

extern "C" int ka_selfplay_state_words(void) { return kSpWords; }
// which: 0 = int32 words of one env's plan, 1 = int64 words of the store descriptor, 2 = int32 words of one truncation
// record, 3 = the largest number of envs
extern "C" int ka_selfplay_layout(int which) {
    return which == 0 ? kSpPlan : which == 1 ? kSpDesc : which == 2 ? kSpTrunc : which == 3 ? kSpMaxEnvs : -1;
}

extern "C" int ka_selfplay_step(int* state, int envs, const float* obs, const void* mask_bits, const long long* actions,
                                const float* logp, const float* vlogits, const float* score_lead, float alpha,
                                const int* nlegal, const void* pre_player, const float* rewards, const void* terminated,
                                const void* truncated, const int* material, float score_norm, const float* term_obs,
                                const long long* refusal, void* stall, float* values, float* t_obs, int* t_list,
                                const long long* desc, int* plan, int obs_elems, int mask_words, void* stream) {
    KA_REQUIRE(state && desc && plan, "selfplay_step: null state, descriptor or plan");
    KA_REQUIRE(obs && mask_bits && actions && logp && vlogits && nlegal && pre_player && rewards && terminated && truncated &&
               material && term_obs && stall && values && t_obs && t_list, "selfplay_step: null tensor");
    KA_REQUIRE(envs > 0 && envs <= kSpMaxEnvs, "selfplay_step: envs %d (1..%d)", envs, kSpMaxEnvs);
    KA_REQUIRE(obs_elems > 0 && mask_words > 0, "selfplay_step: obs_elems %d, mask_words %d", obs_elems, mask_words);
    KA_REQUIRE(score_norm == score_norm && score_norm != 0.f, "selfplay_step: score_norm %f", (double)score_norm);
    SelfPlayArgs a{state, envs, obs, static_cast<const uint32_t*>(mask_bits), actions, logp, vlogits, score_lead, alpha, nlegal,
                   static_cast<const uint8_t*>(pre_player), rewards, static_cast<const uint8_t*>(terminated),
                   static_cast<const uint8_t*>(truncated), material, score_norm, term_obs, refusal,
                   static_cast<uint8_t*>(stall), values, t_obs, t_list, desc, plan, obs_elems, mask_words};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(selfplay_plan_kernel, dim3(1), dim3(kSpThreads), 0, st, a);
    hipLaunchKernelGGL(selfplay_copy_kernel, dim3(envs), dim3(kSpThreads), 0, st, a);
    return ka_check_launch("selfplay_step");
}
