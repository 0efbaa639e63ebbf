// Search samples: the positions the arena's visit-count search looked at, kept inside the ply as training rows
// (keisei_amd/training/search_samples.py; an addition the reference does not have).  MctsSearch leaves the visit counts of a
// searched position for one ply only, and a captured graph gives the host no look in between: this launch, one per ply
// behind the env step and before the referee rewrites model_of, copies them into dataset rows on the device and labels a
// game's rows with its result when the game ends.
//
// Store: per env a region of rows_per_env sample rows of kSsRowWords = 216 dwords (864 bytes):
//   [0, 204)    the packed position, the layout of KA_SL_PACKED_WORDS (sl_data.hip): the observation BEFORE the move, packed
//               by sl_pack_kernel's channel pass; 200 policy = the action stepped (after any mate override), 201 value = -1
//               until the game ends, 202 the bits of (float)material / 76.0f from the step's material balance, 203 zero
//   [204, 212)  visit word j = action | visits << 16 of root candidate j < n_cand, 0 for an unused slot (visits 0 = unused)
//   [212, 216)  info: model | mover << 16, index of the move in its game, env, game number (games the env finished
//               since the host zeroed the meta)
// Meta: per env kSsMeta int32 {write cursor, first row of the game in progress, samples dropped, moves played in the game in
// progress, games finished}.  One error word: bit 0 = an observation that cannot be held packed.
//
// search_sample_kernel is one workgroup per env; an env touches its own region and its own meta words only, thread 0 is the
// only reader and writer of the meta (the other waves get it through LDS, as sl_record_kernel's cursor), and the one atomic
// is the OR into the error word.  It reads the env's PREVIOUS result buffers (the position before the move, intact until
// the step after the next one) and the step's own results.
#include "common.h"
#include "sl_packed.h"

namespace {

constexpr int kSsVisits = 8, kSsInfo = 4, kSsMeta = 5;
constexpr int kSsVisitAt = kPkWords, kSsInfoAt = kSsVisitAt + kSsVisits;
constexpr int kSsRowWords = kSsInfoAt + kSsInfo;              // 216
constexpr int kSsRecFlags = 0, kSsRecNcand = 2, kSsRecCand = 4;    // the search's record (lookahead_record.h): flags bit 0 = active
constexpr int kSsMaxEnvs = 1 << 20;
static_assert(kSsRowWords <= kPkThreads, "one thread per word of the row");

struct SampleArgs {
    const uint32_t* obs; const uint8_t* players;              // the previous buffers: the positions before the move
    const int* records; int rec_words; const int* root_visits; int width;
    const int* model_of; const long long* actions;
    const int* material; const float* rewards; const uint8_t* terminated; const uint8_t* truncated;   // the step's result
    uint32_t* rows; int rows_per_env; int* meta; int* err; int E;
};

__global__ __launch_bounds__(kPkThreads) void search_sample_kernel(SampleArgs a) {
    __shared__ uint32_t s_row[kSsRowWords];
    __shared__ int s_meta[kSsMeta];
    __shared__ int s_bad[kPkWaves];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (e >= a.E) return;
    int* meta = a.meta + (size_t)e * kSsMeta;
    if (tid == 0)
        for (int w = 0; w < kSsMeta; ++w) s_meta[w] = meta[w];
    __syncthreads();
    const int cursor = s_meta[0], first = s_meta[1], moves = s_meta[3], games = s_meta[4];
    const int* rec = a.records + (size_t)e * a.rec_words;
    const int ncand = rec[kSsRecNcand], model = a.model_of[e];
    const bool want = (rec[kSsRecFlags] & 1) != 0 && ncand >= 1 && model >= 0;      // uniform over the workgroup, as all below
    const bool fits = cursor >= 0 && cursor < a.rows_per_env;
    const bool write = want && fits;
    const bool done = a.terminated[e] != 0 || a.truncated[e] != 0;
    const int mover = a.players[e] & 1;
    const float reward = a.rewards[e];
    const int winner = reward > 0.f ? mover : (reward < 0.f ? 1 - mover : 2);     // the game log's rule: a NaN is a draw
    uint32_t* region = a.rows + (size_t)e * a.rows_per_env * kSsRowWords;
    if (write) {
        const bool bad = sl_pack_channels(a.obs + (size_t)e * kPkObsWords, s_row, lane, wave);
        if (lane == 0) s_bad[wave] = bad;
        if (tid == 0) {
            s_row[kPkPolicyAt + 0] = (uint32_t)a.actions[e];
            s_row[kPkPolicyAt + 1] = !done ? 0xffffffffu : (winner == 2 ? 1u : (winner == mover ? 0u : 2u));
            s_row[kPkPolicyAt + 2] = __float_as_uint((float)a.material[e] / 76.0f);
            s_row[kPkPolicyAt + 3] = 0u;
            s_row[kSsInfoAt + 0] = (uint32_t)model | ((uint32_t)mover << 16);
            s_row[kSsInfoAt + 1] = (uint32_t)moves;
            s_row[kSsInfoAt + 2] = (uint32_t)e;
            s_row[kSsInfoAt + 3] = (uint32_t)games;
        }
        if (tid >= 64 && tid < 64 + kSsVisits) {                // (a wave other than thread 0's)
            const int j = tid - 64;
            uint32_t word = 0u;
            if (j < ncand && j < a.width) {
                const int visits = a.root_visits[(size_t)e * a.width + j];
                if (visits > 0) word = ((uint32_t)rec[kSsRecCand + j] & 0xffffu) | (((uint32_t)visits & 0xffffu) << 16);
            }
            s_row[kSsVisitAt + j] = word;
        }
        __syncthreads();
        if (tid < kSsRowWords) region[(size_t)cursor * kSsRowWords + tid] = s_row[tid];
        if (tid == 0 && (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) != 0) atomicOr(a.err, 1);
    }
    if (done) {                                                // the game's earlier rows: written by launches before this one
        const int last = min(cursor, a.rows_per_env);
        for (int r = max(first, 0) + tid; r < last; r += kPkThreads) {
            uint32_t* row = region + (size_t)r * kSsRowWords;
            const int m = (int)(row[kSsInfoAt] >> 16) & 1;
            row[kPkPolicyAt + 1] = winner == 2 ? 1u : (m == winner ? 0u : 2u);
        }
    }
    if (tid == 0) {
        const int next = cursor + (write ? 1 : 0);
        meta[0] = next;
        meta[1] = done ? next : first;
        meta[2] = s_meta[2] + (want && !fits ? 1 : 0);
        meta[3] = done ? 0 : moves + 1;
        meta[4] = games + (done ? 1 : 0);
    }
}

}  // namespace

// which: 0 = words of a sample row, 1 = meta words per env, 2 = visit words, 3 = info words, 4 = the largest number of envs
extern "C" int ka_search_sample_words(int which) {
    return which == 0 ? kSsRowWords : which == 1 ? kSsMeta : which == 2 ? kSsVisits : which == 3 ? kSsInfo
         : which == 4 ? kSsMaxEnvs : -1;
}

extern "C" int ka_search_sample_step(const float* obs_prev, int obs_elems, const void* players_prev, const int* records,
                                     int rec_words, const int* root_visits, int width, const int* model_of,
                                     const long long* actions, const int* material, const float* rewards,
                                     const void* terminated, const void* truncated, void* rows, int rows_per_env, int* meta,
                                     int* err, int envs, void* stream) {
    KA_REQUIRE(obs_prev && players_prev && records && root_visits && model_of && actions && material && rewards &&
               terminated && truncated && rows && meta && err, "search_sample_step: null tensor");
    KA_REQUIRE(envs > 0 && envs <= kSsMaxEnvs, "search_sample_step: envs %d (1..%d)", envs, kSsMaxEnvs);
    KA_REQUIRE(obs_elems == kPkObsWords, "search_sample_step: obs_elems %d (a packed position holds %d)", obs_elems, kPkObsWords);
    KA_REQUIRE(width >= 1 && width <= kSsVisits, "search_sample_step: width %d (1..%d)", width, kSsVisits);
    KA_REQUIRE(rec_words >= kSsRecCand + width, "search_sample_step: records of %d words (at least %d)", rec_words,
               kSsRecCand + width);
    KA_REQUIRE(rows_per_env >= 1 && (long long)envs * rows_per_env * kSsRowWords < (1ll << 40),
               "search_sample_step: rows_per_env %d", rows_per_env);
    KA_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 3) == 0 && (reinterpret_cast<uintptr_t>(obs_prev) & 3) == 0,
               "search_sample_step: the rows and the observations must be 4-byte aligned");
    SampleArgs a{reinterpret_cast<const uint32_t*>(obs_prev), static_cast<const uint8_t*>(players_prev), records, rec_words,
                 root_visits, width, model_of, actions, material, rewards, static_cast<const uint8_t*>(terminated),
                 static_cast<const uint8_t*>(truncated), static_cast<uint32_t*>(rows), rows_per_env, meta, err, envs};
    hipLaunchKernelGGL(search_sample_kernel, dim3(envs), dim3(kPkThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("search_sample_step");
}
