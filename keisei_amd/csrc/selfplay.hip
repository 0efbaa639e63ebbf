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
// State: ka_selfplay_state_words() int32, read by the host in one copy.  The words shared with the league step are
// tabulated in rollout_rows.h (the tallies are in the mover's frame); self-play's own:
//   2     ply of the epoch: the p of the row rule.  The kernel advances it, the host zeroes it when a collect begins
//   4     plies stepped since the last reset (the host never clears it between resets)
//   25    an env had no legal action (the envs are latched in `stall`)
//   10-11, 26-31 unused
#include "rollout_rows.h"

namespace {

constexpr int kSpThreads = 256;
constexpr int kSpWords = 32, kSpPlan = 2, kSpTrunc = 2;
enum { kPly = 2, kPlies = 4, kStall = 25 };                    // self-play's own state words

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
    Columns c = load_columns(a.desc);
    c.env_ids = nullptr;                                       // the dense layout has no such column: the pointer is not read
    const int ply = st[kPly], tfirst = st[kTrunc];
    const long long first = (long long)ply * E;               // this ply's first row behind the base row

    int runt = 0;
    int stall = 0, written = 0, dropped = 0, tdropped = 0;
    Tallies tl{};
    RowGuards g{0, 0, 0, 0};
    for (int tile = 0; tile < E; tile += kSpThreads) {
        const int k = tile + tid;
        const bool have = k < E;
        const bool tm = have && a.terminated[k] != 0;
        const bool done = have && (tm || a.truncated[k] != 0);  // :1458
        const bool trunc_only = done && !tm;                    // :1502
        const bool fits = have && first + k < c.cap;
        int t;
        runt += ka_tile_rank(trunc_only && fits, runt, wsum, &t);
        if (!have) continue;
        const float r = a.rewards[k];                           // the mover's frame: no flip in this branch
        const int pre = a.pre_player[k] & 1;
        // tallies (:1460-1485)
        tally_add(tl, tm, trunc_only, r, r, pre);
        if (a.nlegal[k] == 0) { stall = 1; a.stall[k] = 1; }
        const float value = ka_blended_value(a.vlogits + k * 3, a.score_lead ? a.score_lead + k : nullptr, a.alpha);
        a.values[k] = value;                                    // :1446, latest_values
        int* plan = a.plan + (size_t)k * kSpPlan;
        if (!fits) {
            dropped += 1;
            plan[0] = -1; plan[1] = -1;
            continue;
        }
        // the row's scalar columns (:1487-1527)
        const long long row = c.base + first + k;
        write_row(c, row, k, a.actions[k], a.logp[k], value, r, done, tm, (float)a.material[k] / a.score_norm, true, &g);
        written += 1;
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
    commit_tallies_and_guards<T>(tl, g, st, red);
    written = ka_block_sum<T>(written, red); dropped = ka_block_sum<T>(dropped, red); tdropped = ka_block_sum<T>(tdropped, red);
    stall = ka_block_max<T>(stall, red);
    if (tid == 0) {
        ply_tail(st, kRefusal, a.refusal);
        st[kPly] = ply + 1;
        st[kPlies] += 1;
        st[kRows] += written;
        st[kDropped] += dropped;
        st[kTrunc] = min(E, tfirst + runt);
        st[kTruncDropped] += tdropped;
        st[kStall] |= stall;
    }
}

__global__ __launch_bounds__(kSpThreads) void selfplay_copy_kernel(SelfPlayArgs a) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const long long row = a.plan[(size_t)e * kSpPlan];
    const int ts = a.plan[(size_t)e * kSpPlan + 1];
    if (row < 0) return;                                        // (a truncation slot always comes with a row)
    const size_t n = a.obs_elems;
    const Columns c = load_columns(a.desc);
    copy_transition<kSpThreads>(c.obs, c.bits, row, a.obs, a.bits, e, a.obs_elems, a.words);
    if (ts >= 0) ka_copy_row<kSpThreads>(a.t_obs + ts * n, a.term_obs + e * n, a.obs_elems, tid);
}

}  // namespace

extern "C" int ka_selfplay_state_words(void) { return kSpWords; }
// which: 0 = int32 words of one env's plan, 1 = int64 words of the store descriptor, 2 = int32 words of one truncation
// record, 3 = the largest number of envs
extern "C" int ka_selfplay_layout(int which) {
    return which == 0 ? kSpPlan : which == 1 ? kRolloutDesc : which == 2 ? kSpTrunc : which == 3 ? kRolloutMaxEnvs : -1;
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
    KA_REQUIRE_ROLLOUT_STEP("selfplay_step", envs, obs_elems, mask_words, score_norm);
    SelfPlayArgs a{state, envs, obs, static_cast<const uint32_t*>(mask_bits), actions, logp, vlogits, score_lead, alpha, nlegal,
                   static_cast<const uint8_t*>(pre_player), rewards, static_cast<const uint8_t*>(terminated),
                   static_cast<const uint8_t*>(truncated), material, score_norm, term_obs, refusal,
                   static_cast<uint8_t*>(stall), values, t_obs, t_list, desc, plan, obs_elems, mask_words};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(selfplay_plan_kernel, dim3(1), dim3(kSpThreads), 0, st, a);
    hipLaunchKernelGGL(selfplay_copy_kernel, dim3(envs), dim3(kSpThreads), 0, st, a);
    return ka_check_launch("selfplay_step");
}
