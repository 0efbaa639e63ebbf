// SL shard preparation: game records replayed on the device (the work keisei/sl/prepare.py:151-161 lists and leaves out:
// replay the moves, observe every position, encode the played move, take the material balance).  The host turns a batch of E
// records into one stream of spatial action indices; game g sits in env g, all envs step in lockstep from ka_shogi_env_reset.
// One ply is three launches on one stream, with no host read:
//   sl_plan_kernel     ONE workgroup, tiles of 256 envs.  Tests the record's move against the packed mask row of the
//                      position to move and hands the env step a legal action for EVERY env: the record's move where the
//                      game is live and the move legal (write = 1), the lowest legal action otherwise (write = 0) -- the env
//                      step refuses the whole batch for one illegal action, and there is no idle action.  It is the only
//                      writer of the counters.
//   ka_shogi_env_step  unchanged (csrc/shogi_env.hip)
//   sl_record_kernel   one workgroup per env.  If write: the 16 220-byte shard record {f32 obs[4050], i64 policy, i64 value,
//                      f32 score} into row row_of[g] + i, from the env's PREVIOUS result buffer (the position before the
//                      move, intact until the step after the next one).  Then the env's own words: a game the rules ended
//                      before its record did is cut (the env has restarted it), the cursor advances.
// A record row starts at 16 220 * r bytes: 4-byte aligned, 8-byte aligned only for even r.  Every store to the shard buffer
// is a 4-byte store, the two int64 targets as two dwords each.
//
// State: int32, ka_sl_replay_state_words(0) header words, then three arrays of E words: cursor, valid_len, reason.
//   0     plies planned since the host zeroed the header
//   1     records written (write = 1)
//   2     filler steps (write = 0)
//   3     games cut at an illegal move
//   4     games cut because the rules ended them before the record did (counted at the ply after the cut)
//   5     envs without any legal action (the env step will refuse: the host raises)
//   6-7   copy of the VecEnv refusal latch (int64) after the latest step
// A game is live while cursor < valid_len; the host sets valid_len = len.  reason: 0 none, 1 illegal move, 2 ended by the rules.
#include "common.h"

namespace {

constexpr int kSlThreads = 256;
constexpr int kSlWords = 8;
constexpr int kSlMaxEnvs = 4096;
constexpr int kSlRowWords = 4055;                              // 16 220 B
constexpr int kSlObsWords = 4050;
constexpr int kSlActions = 81 * 139;
constexpr int kSlMaskWords = (kSlActions + 31) / 32;
enum { kSlPlies = 0, kSlWritten = 1, kSlFiller = 2, kSlIllegal = 3, kSlRules = 4, kSlStall = 5, kSlRefusal = 6 };
enum { kReasonNone = 0, kReasonIllegal = 1, kReasonRules = 2 };

struct SlArgs {
    int* state; int E;
    const int* actions; int total;                             // the batch's action stream
    const int* offset; const int* outcome; const int* row_of;
    const uint32_t* bits;                                      // packed masks of the positions to move
    long long* act; int* write;
    // the record kernel
    const uint32_t* obs; const uint8_t* players;               // the previous buffers: the positions before the move
    const int* material; const uint8_t* terminated; const uint8_t* truncated;    // the step's result
    const long long* refusal;
    uint32_t* shard; int rows;
};

__global__ __launch_bounds__(kSlThreads) void sl_plan_kernel(SlArgs a) {
    __shared__ int red[kSlThreads / 64];
    const int tid = threadIdx.x, E = a.E;
    int* st = a.state;
    int* cursor = st + kSlWords;
    int* valid_len = cursor + E;
    int* reason = valid_len + E;
    int written = 0, filler = 0, illegal = 0, rules = 0, stall = 0;
    for (int tile = 0; tile < E; tile += kSlThreads) {
        const int k = tile + tid;
        if (k >= E) continue;
        const int i = cursor[k], vl = valid_len[k];
        const uint32_t* row = a.bits + (size_t)k * kSlMaskWords;
        rules += reason[k] == kReasonRules && vl == i;          // cut by the record kernel of the ply before
        const long long at = (long long)a.offset[k] + i;
        const bool live = i < vl && at >= 0 && at < a.total;
        int mv = live ? a.actions[at] : -1;
        const bool legal = live && mv >= 0 && mv < kSlActions && ((row[mv >> 5] >> (mv & 31)) & 1u);
        if (live && !legal) { valid_len[k] = i; reason[k] = kReasonIllegal; illegal += 1; }
        if (!legal) {
            mv = -1;
            for (int w = 0; w < kSlMaskWords; ++w) {
                const uint32_t word = row[w];
                if (word) { mv = w * 32 + __ffs(word) - 1; break; }
            }
            if (mv < 0) { mv = 0; stall += 1; }
        }
        a.act[k] = mv;
        a.write[k] = legal;
        written += legal; filler += !legal;
    }
    constexpr int T = kSlThreads;
    written = ka_block_sum<T>(written, red); filler = ka_block_sum<T>(filler, red); illegal = ka_block_sum<T>(illegal, red);
    rules = ka_block_sum<T>(rules, red); stall = ka_block_sum<T>(stall, red);
    if (tid == 0) {
        st[kSlPlies] += 1; st[kSlWritten] += written; st[kSlFiller] += filler; st[kSlIllegal] += illegal;
        st[kSlRules] += rules; st[kSlStall] += stall;
    }
}

__global__ __launch_bounds__(kSlThreads) void sl_record_kernel(SlArgs a) {
    __shared__ int s_cursor;
    const int e = blockIdx.x, tid = threadIdx.x, E = a.E;
    int* cursor = a.state + kSlWords;
    int* valid_len = cursor + E;
    int* reason = valid_len + E;
    // thread 0 is the only reader and writer of cursor[e], valid_len[e] and reason[e] in this kernel: the other waves get
    // the cursor through LDS, so a wave that starts late cannot see the advanced one
    if (tid == 0) s_cursor = cursor[e];
    __syncthreads();
    const int i = s_cursor;
    const long long r = (long long)a.row_of[e] + i;
    const bool write = a.write[e] != 0 && r >= 0 && r < a.rows;
    if (write) {
        uint32_t* dst = a.shard + (size_t)r * kSlRowWords;
        const uint32_t* src = a.obs + (size_t)e * kSlObsWords;
        for (int j = tid; j < kSlObsWords; j += kSlThreads) dst[j] = src[j];
        if (tid == 0) {
            const int mover = a.players[e] & 1, out = a.outcome[e];     // outcome: 0 black wins, 1 white wins, 2 draw
            const uint32_t value = out == 2 ? 1u : (out == mover ? 0u : 2u);
            dst[kSlObsWords + 0] = (uint32_t)a.act[e]; dst[kSlObsWords + 1] = 0u;
            dst[kSlObsWords + 2] = value; dst[kSlObsWords + 3] = 0u;
            dst[kSlObsWords + 4] = __float_as_uint((float)a.material[e] / 76.0f);
        }
    }
    if (tid == 0) {
        const bool done = a.terminated[e] != 0 || a.truncated[e] != 0;
        if (a.write[e] != 0 && done && i + 1 < valid_len[e]) { valid_len[e] = i + 1; reason[e] = kReasonRules; }
        cursor[e] = i + 1;
        if (e == 0 && a.refusal) {
            const unsigned long long w = (unsigned long long)*a.refusal;
            a.state[kSlRefusal] = (int)(uint32_t)w; a.state[kSlRefusal + 1] = (int)(uint32_t)(w >> 32);
        }
    }
}

}  // namespace

// which: 0 = header words, 1 = words per env behind the header, 2 = the largest number of envs, 3 = bytes of a shard record
extern "C" int ka_sl_replay_state_words(int which) {
    return which == 0 ? kSlWords : which == 1 ? 3 : which == 2 ? kSlMaxEnvs : which == 3 ? kSlRowWords * 4 : -1;
}

extern "C" int ka_sl_replay_plan(int* state, int envs, const int* actions, int total, const int* offset,
                                 const void* mask_bits, int mask_words, long long* act, int* write, void* stream) {
    KA_REQUIRE(state && actions && offset && mask_bits && act && write, "sl_replay_plan: null tensor");
    KA_REQUIRE(envs > 0 && envs <= kSlMaxEnvs, "sl_replay_plan: envs %d (1..%d)", envs, kSlMaxEnvs);
    KA_REQUIRE(total > 0, "sl_replay_plan: empty action stream (%d)", total);
    KA_REQUIRE(mask_words == kSlMaskWords, "sl_replay_plan: mask_words %d (the spatial action space packs into %d)", mask_words,
               kSlMaskWords);
    SlArgs a{};
    a.state = state; a.E = envs; a.actions = actions; a.total = total; a.offset = offset;
    a.bits = static_cast<const uint32_t*>(mask_bits); a.act = act; a.write = write;
    hipLaunchKernelGGL(sl_plan_kernel, dim3(1), dim3(kSlThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("sl_replay_plan");
}

extern "C" int ka_sl_replay_record(int* state, int envs, const int* outcome, const int* row_of, const float* obs,
                                   int obs_elems, const void* players, const long long* act, const int* write,
                                   const int* material, const void* terminated, const void* truncated,
                                   const long long* refusal, void* shard, int rows, void* stream) {
    KA_REQUIRE(state && outcome && row_of && obs && players && act && write && material && terminated && truncated && shard,
               "sl_replay_record: null tensor");
    KA_REQUIRE(envs > 0 && envs <= kSlMaxEnvs, "sl_replay_record: envs %d (1..%d)", envs, kSlMaxEnvs);
    KA_REQUIRE(obs_elems == kSlObsWords, "sl_replay_record: obs_elems %d (a shard record holds %d)", obs_elems, kSlObsWords);
    KA_REQUIRE(rows > 0, "sl_replay_record: rows %d", rows);
    KA_REQUIRE((reinterpret_cast<uintptr_t>(shard) & 3) == 0 && (reinterpret_cast<uintptr_t>(obs) & 3) == 0,
               "sl_replay_record: the shard buffer and the observations must be 4-byte aligned");
    SlArgs a{};
    a.state = state; a.E = envs; a.outcome = outcome; a.row_of = row_of; a.obs = reinterpret_cast<const uint32_t*>(obs);
    a.players = static_cast<const uint8_t*>(players); a.act = const_cast<long long*>(act); a.write = const_cast<int*>(write);
    a.material = material; a.terminated = static_cast<const uint8_t*>(terminated);
    a.truncated = static_cast<const uint8_t*>(truncated); a.refusal = refusal;
    a.shard = static_cast<uint32_t*>(shard); a.rows = rows;
    hipLaunchKernelGGL(sl_record_kernel, dim3(envs), dim3(kSlThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("sl_replay_record");
}
