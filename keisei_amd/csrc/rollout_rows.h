// The PPO rows the step kernels of a rollout write on the device, stated once: the store descriptor, the shared state words,
// the scalar columns of one transition with the store's input guards, the tallies, the tail of a ply and the copy of a
// transition's big rows.  The league step (csrc/league.hip) and the self-play step (csrc/selfplay.hip) take all of it; the
// arena (csrc/arena.hip) takes the ply's tail for its referee and the transition copy for record_pre.
#pragma once
#include "common.h"

constexpr int kRolloutMaxEnvs = 4096;
// The store descriptor: kRolloutDesc int64 words on the device, rewritten by the host at each sync point, in the order of
// Columns.  training/_device_ply.py's _DESC_KEYS is the Python mirror of the twelve column pointers (a column the store
// does not have is 0); base is the base row, cap the rows reserved behind it.
constexpr int kRolloutDesc = 14;
struct Columns {
    float* obs; uint32_t* bits; long long* actions; float* logp; float* values; float* rewards; uint8_t* dones;
    uint8_t* terminated; long long* cats; float* score; long long* env_ids; float* override_;
    long long base, cap;
};
static_assert(sizeof(Columns) == kRolloutDesc * sizeof(long long), "Columns is the descriptor, word for word");
__device__ __forceinline__ Columns load_columns(const long long* desc) { return *reinterpret_cast<const Columns*>(desc); }

// The int32 words of the state array that mean the same in both step kernels (training/_device_ply.py reads them by these
// numbers); each kernel's own words are in its file.
//   0-1   seed (int64) ka_policy_sample_play reads this ply; advanced by a Weyl step per ply
//   3     rows written behind the descriptor's base row
//   5     rows that did not fit the reserved capacity
//   6-7   the sampler's flags [NaN logits, a row without a legal action]
//   8-9   copy of the VecEnv refusal latch (int64)
//   12    truncation slots used since the host last cleared it
//   13    truncation records that found no slot
//   14-20 wins, losses, draws (the frame is the kernel's), black wins, white wins, terminated, truncated-only
//   21-24 the rollout store's input guards over the rows written: terminated without done, value category outside
//         {-1, 0, 1, 2}, NaN score target, bits of max |score target|  (ka_rollout_append's four flags)
enum { kSeed = 0, kRows = 3, kDropped = 5, kSamp = 6, kRefusal = 8, kTrunc = 12, kTruncDropped = 13, kTallies = 14, kGuards = 21 };

// the value-head label of a transition (_compute_value_cats, katago_loop.py:75-92): only terminated rows get one; 3, a NaN
// reward, is what the bad-category guard catches
__device__ __forceinline__ long long rollout_value_cat(bool term, float reward) {
    return !term ? -1 : (reward > 0.f ? 0 : (reward == 0.f ? 1 : (reward < 0.f ? 2 : 3)));
}

// the store's four input guards over the rows one thread wrote
struct RowGuards { int term_not_done, bad_cat, nan_score, peak; };
// one transition's scalar columns (katago_loop.py:1299-1316 / :1347-1365 / :1487-1527); label = false leaves the row
// without a value category (the league's flush)
__device__ __forceinline__ void write_row(const Columns& c, long long row, int env, long long action, float logp, float value,
                                          float reward, bool done, bool term, float score, bool label, RowGuards* g) {
    const long long cat = rollout_value_cat(label && term, reward);
    c.actions[row] = action; c.logp[row] = logp; c.values[row] = value; c.rewards[row] = reward;
    c.dones[row] = done; c.terminated[row] = term; c.cats[row] = cat; c.score[row] = score;
    if (c.env_ids) c.env_ids[row] = env;                       // (self-play's dense (T, N) layout has no such column)
    c.override_[row] = __uint_as_float(0x7fc00000u);           // NaN: the host fills the truncated rows at the sync point
    g->term_not_done |= term && !done;
    g->bad_cat |= cat < -1 || cat > 2;
    if (score != score) g->nan_score = 1;
    else g->peak = max(g->peak, __float_as_int(fabsf(score)));
}

// the seven tallies of words 14-20, in that order (katago_loop.py:1219-1248 / :1460-1485).  Wins, losses and draws go by
// the reward in the kernel's frame, black and white wins by the mover's raw reward and the player who moved.
struct Tallies { int n[7]; };
__device__ __forceinline__ void tally_add(Tallies& t, bool tm, bool trunc_only, float frame_reward, float raw_reward, int pre) {
    t.n[5] += tm; t.n[6] += trunc_only;
    if (!tm) return;
    t.n[0] += frame_reward > 0.f; t.n[1] += frame_reward < 0.f; t.n[2] += frame_reward == 0.f;
    t.n[3] += (raw_reward > 0.f && pre == 0) || (raw_reward < 0.f && pre == 1);
    t.n[4] += (raw_reward > 0.f && pre == 1) || (raw_reward < 0.f && pre == 0);
}

// the workgroup's tallies and guards into the state: eleven block reductions (every thread calls it), then thread 0 adds
// the tallies to words 14-20 and latches the guards into words 21-24
template <int THREADS> __device__ __forceinline__ void commit_tallies_and_guards(Tallies t, RowGuards g, int* st, int* red) {
#pragma unroll
    for (int i = 0; i < 7; ++i) t.n[i] = ka_block_sum<THREADS>(t.n[i], red);
    g.term_not_done = ka_block_max<THREADS>(g.term_not_done, red); g.bad_cat = ka_block_max<THREADS>(g.bad_cat, red);
    g.nan_score = ka_block_max<THREADS>(g.nan_score, red); g.peak = ka_block_max<THREADS>(g.peak, red);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int i = 0; i < 7; ++i) st[kTallies + i] += t.n[i];
    st[kGuards + 0] |= g.term_not_done; st[kGuards + 1] |= g.bad_cat; st[kGuards + 2] |= g.nan_score;
    st[kGuards + 3] = max(st[kGuards + 3], g.peak);
}

// the tail of a ply, by one thread: the next ply's sampler seed (a Weyl step; the sampler mixes it) and the env's refusal
// latch, copied so that the host sees a refused step in the same read
__device__ __forceinline__ void ply_tail(int* state, int refusal_word, const long long* refusal) {
    *reinterpret_cast<unsigned long long*>(state) += kKaWeyl;
    if (refusal) *reinterpret_cast<long long*>(state + refusal_word) = *refusal;
}

// the big rows of one transition, by a workgroup of THREADS threads: observation row srow of src_obs and packed mask row
// srow of src_bits to row drow of dst_obs / dst_bits
template <int THREADS>
__device__ __forceinline__ void copy_transition(float* dst_obs, uint32_t* dst_bits, size_t drow, const float* src_obs,
                                                const uint32_t* src_bits, size_t srow, int obs_elems, int words) {
    ka_copy_row<THREADS>(dst_obs + drow * obs_elems, src_obs + srow * obs_elems, obs_elems, threadIdx.x);
    for (int i = threadIdx.x; i < words; i += THREADS) dst_bits[drow * words + i] = src_bits[srow * words + i];
}

// the launchers' common checks, under the entry point's own name (host side)
#define KA_REQUIRE_ROLLOUT_STEP(who, envs, obs_elems, mask_words, score_norm)                                           \
    do {                                                                                                                \
        KA_REQUIRE((envs) > 0 && (envs) <= kRolloutMaxEnvs, who ": envs %d (1..%d)", (envs), kRolloutMaxEnvs);           \
        KA_REQUIRE((obs_elems) > 0 && (mask_words) > 0, who ": obs_elems %d, mask_words %d", (obs_elems), (mask_words)); \
        KA_REQUIRE((score_norm) == (score_norm) && (score_norm) != 0.f, who ": score_norm %f", (double)(score_norm));    \
    } while (0)
