// Match arena: the league-play referee on the device (reference: keisei/training/concurrent_matches.py:196-545,
// ConcurrentMatchPool.run_round).  The envs of one VecEnv are split into S contiguous slots of E envs each (env b belongs
// to slot b / E, partition_range), and every slot plays one pairing (model a as player 0, model b as player 1) until it
// has completed its target number of games.  One ply is: grouped forward on model_of -> ka_policy_sample_play ->
// ka_shogi_env_step -> ka_arena_referee; the host looks at the state only every few plies.
//
// State: one int32 array per arena, read by the host in one copy.
//   words 0-1  seed (int64): the seed ka_policy_sample_play reads this ply; the referee advances it
//   word  2    round ply counter
//   word  3    max_ply of the ply ceiling (set by the host per round)
//   words 4-5  the sampler's flags: [NaN logits, a row without a legal action] (latched, never cleared here)
//   words 6-7  copy of the VecEnv refusal latch (int64), so the host sees a refused step in the same read
//   then S slots of 8 words: model_a, model_b, target, a_wins, b_wins, draws, plies, status
// status bits: 1 = a pairing is seated, 2 = done, 4 = partial (ply ceiling), 8 = stalled (a seated env had no legal action)
//
// ka_arena_referee: one workgroup per slot, so the per-slot counters need no atomics.
#include "rollout_rows.h"

namespace {

constexpr int kArenaThreads = 256;
constexpr int kHdrWords = 8, kSlotWords = 8;
constexpr int kSeated = 1, kDone = 2, kPartial = 4, kStalled = 8;

struct RefereeArgs {
    int* state; int E;
    const float* rewards; const uint8_t* terminated; const uint8_t* truncated; const uint8_t* players;
    const int* nlegal; const long long* refusal; int* model_of; uint8_t* pre_player;
};

__global__ __launch_bounds__(kArenaThreads) void arena_referee_kernel(RefereeArgs a) {
    __shared__ int red[kArenaThreads / 64];
    __shared__ int s_status;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int e0 = s * a.E, e1 = e0 + a.E;
    int* st = a.state + kHdrWords + s * kSlotWords;
    if (s == 0 && tid == 0) {
        ply_tail(a.state, 6, a.refusal);
        a.state[2] += 1;
    }
    const int status = st[7];
    if ((status & kSeated) && !(status & kDone)) {              // uniform over the workgroup
        // concurrent_matches.py:452-469: rewards are the last mover's; the mover was A when its pre-step player was 0
        int aw = 0, bw = 0, dr = 0, stalled = 0;
        for (int e = e0 + tid; e < e1; e += kArenaThreads) {
            stalled |= a.nlegal[e] == 0;
            if (a.terminated[e] || a.truncated[e]) {
                const float r = a.rewards[e];
                const bool a_moved = a.pre_player[e] == 0;
                if (r > 0.f) (a_moved ? aw : bw) += 1;
                else if (r < 0.f) (a_moved ? bw : aw) += 1;
                else dr += 1;
            }
        }
        aw = ka_block_sum<kArenaThreads>(aw, red);
        bw = ka_block_sum<kArenaThreads>(bw, red);
        dr = ka_block_sum<kArenaThreads>(dr, red);
        stalled = ka_block_sum<kArenaThreads>(stalled, red);
        if (tid == 0) {
            int ns = status;
            const int plies = st[6] + 1;
            st[6] = plies;
            if (stalled) {                                      // :291-302: the slot is not tallied; target = games so far
                st[2] = st[3] + st[4] + st[5];
                ns |= kDone | kStalled;
            } else {
                st[3] += aw; st[4] += bw; st[5] += dr;
                const int target = st[2];
                if (st[3] + st[4] + st[5] >= target) {
                    ns |= kDone;                                // every completion of this ply counts (overshoot)
                } else {
                    const long long waves = (target + a.E - 1) / a.E;         // :473-486
                    if ((long long)plies >= (long long)a.state[3] * (waves + 1)) ns |= kDone | kPartial;
                }
            }
            st[7] = ns;
            s_status = ns;
        }
        __syncthreads();
    } else if (tid == 0) {
        s_status = status;
    }
    __syncthreads();
    // seat the next ply: player 0 -> model a, player 1 -> model b; envs of idle or finished slots are unseated
    const int ns = s_status;
    const bool live = (ns & kSeated) && !(ns & kDone);
    const int ma = st[0], mb = st[1];
    for (int e = e0 + tid; e < e1; e += kArenaThreads) {
        if (live) {
            const uint8_t p = a.players[e];
            a.model_of[e] = p == 0 ? ma : mb;
            a.pre_player[e] = p;
        } else {
            a.model_of[e] = -1;
        }
    }
}

// jobs: n rows of {slot, model_a, model_b, target}; one workgroup per job
__global__ __launch_bounds__(kArenaThreads) void arena_assign_kernel(int* state, const int* jobs, int E, const uint8_t* players,
                                                                     int* model_of, uint8_t* pre_player) {
    const int* j = jobs + blockIdx.x * 4;
    const int s = j[0], ma = j[1], mb = j[2];
    if (threadIdx.x == 0) {
        int* st = state + kHdrWords + s * kSlotWords;
        st[0] = ma; st[1] = mb; st[2] = j[3];
        st[3] = 0; st[4] = 0; st[5] = 0; st[6] = 0;
        st[7] = kSeated;
    }
    for (int e = s * E + threadIdx.x; e < (s + 1) * E; e += kArenaThreads) {
        const uint8_t p = players[e];
        model_of[e] = p == 0 ? ma : mb;
        pre_player[e] = p;
    }
}

// ---- rollout collection (concurrent_matches.py:80-163, 318-432: the per-slot _obs / _masks / _perspective / _actions /
// _rewards / _dones lists).  The store is one region of `cap` rows per slot; row r of slot s is store row s * cap + r.
// cursors: 4 int32 per slot {rows committed, rows written this ply, rows dropped, unused}.  A ply's rows are written by
// record_pre at rows committed + rank and committed by record_post, so every workgroup of record_pre reads the same
// cursor and the order inside a slot is (ply, env) whatever the arrival order of the workgroups.
constexpr int kCursorWords = 4;

struct RecordPreArgs {
    const int* state; const int* side_bits; int E;
    const float* obs; const uint32_t* mask; const long long* actions; const uint8_t* pre_player; const int* nlegal;
    int* cursors; int* row_of;
    float* st_obs; uint32_t* st_mask; long long* st_actions; uint8_t* st_persp;
    int cap; int obs_elems; int mask_words;
};

// grid (slots, Y): every workgroup of a slot repeats the slot's scan over its E envs (E bytes and E words), workgroup y
// then copies the rows of envs y, y + Y, ...; workgroup 0 alone writes row_of and the slot's counters.
__global__ __launch_bounds__(kArenaThreads) void arena_record_pre_kernel(RecordPreArgs a) {
    extern __shared__ int s_rank[];                            // E ints: rank of the env's row this ply, -1 = no row
    __shared__ int red[kArenaThreads / 64];
    __shared__ int wsum[kArenaThreads / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int e0 = s * a.E;
    const int status = a.state[kHdrWords + s * kSlotWords + 7];
    const int bits = a.side_bits[s];
    bool live = (status & kSeated) && !(status & kDone) && (bits & 3);      // uniform over the workgroup
    if (live) {
        int stalled = 0;
        for (int k = tid; k < a.E; k += kArenaThreads) stalled |= a.nlegal[e0 + k] == 0;
        live = ka_block_sum<kArenaThreads>(stalled, red) == 0; // :303-314: a slot with a zero-legal env appends nothing
    }
    if (!live) {
        if (blockIdx.y == 0) {
            for (int k = tid; k < a.E; k += kArenaThreads) a.row_of[e0 + k] = -1;
            if (tid == 0) a.cursors[s * kCursorWords + 1] = 0;
        }
        return;
    }
    int running = 0;
    for (int base = 0; base < a.E; base += kArenaThreads) {
        const int k = base + tid;
        const bool want = k < a.E && ((bits >> (a.pre_player[e0 + k] & 1)) & 1);
        int rank;
        const int tot = ka_tile_rank(want, running, wsum, &rank);
        if (k < a.E) s_rank[k] = rank;
        running += tot;
    }
    __syncthreads();
    const int first = a.cursors[s * kCursorWords + 0];
    const int room = max(0, a.cap - first);                    // rows of this ply that still fit
    if (blockIdx.y == 0) {
        for (int k = tid; k < a.E; k += kArenaThreads) {
            const int r = s_rank[k];
            a.row_of[e0 + k] = (r >= 0 && r < room) ? s * a.cap + first + r : -1;
        }
        if (tid == 0) {
            a.cursors[s * kCursorWords + 1] = min(running, room);
            a.cursors[s * kCursorWords + 2] += max(0, running - room);
        }
    }
    for (int k = blockIdx.y; k < a.E; k += gridDim.y) {
        const int r = s_rank[k];
        if (r < 0 || r >= room) continue;
        const size_t row = (size_t)s * a.cap + first + r, e = (size_t)(e0 + k);
        // (the launcher holds the rows to an even length and 8-byte alignment, so the copy goes in 8-byte vectors)
        copy_transition<kArenaThreads>(a.st_obs, a.st_mask, row, a.obs, a.mask, e, a.obs_elems, a.mask_words);
        if (tid == 0) {
            a.st_actions[row] = a.actions[e];
            a.st_persp[row] = a.pre_player[e];
        }
    }
}

__global__ __launch_bounds__(kArenaThreads) void arena_record_post_kernel(int* cursors, const int* row_of, int E, const float* rewards,
                                                                         const uint8_t* terminated, const uint8_t* truncated,
                                                                         float* st_rewards, float* st_dones, int total_rows) {
    const int s = blockIdx.x, e0 = s * E;
    for (int k = threadIdx.x; k < E; k += kArenaThreads) {
        const int r = row_of[e0 + k];
        if (r < 0 || r >= total_rows) continue;
        st_rewards[r] = rewards[e0 + k];
        st_dones[r] = (terminated[e0 + k] || truncated[e0 + k]) ? 1.f : 0.f;
    }
    if (threadIdx.x == 0) {                                    // commit the ply's rows
        cursors[s * kCursorWords + 0] += cursors[s * kCursorWords + 1];
        cursors[s * kCursorWords + 1] = 0;
    }
}

// ---- per-game style features (game_feature_tracker.py:176-356, the GameFeatureTracker every slot gets at seat time,
// concurrent_matches.py:125-130, and feeds every stepped ply, :441-452).
// acc: kAccWords int32 per env = {opening actions kept, num_repetitions, 12 opening actions, side A, side B}; a side is
//   {first_capture_ply, first_drop_ply, num_captures, num_drops, num_promotions, num_early_drops, rook_moved_ply,
//    rook_moves_in_20, king_displacement_20, king_moves_in_30} (_SideStats order), -1 where the reference holds None.
// records: `cap` game records per slot, kRecWords int32 each = {env, total plies, termination reason, last mover, reward
//   sign, opening actions kept, num_repetitions, round ply, 12 opening actions, side A, side B}: one per finished GAME, the
//   host expands it into the black and the white row.
// fcursors: kFeatCursorWords int32 per slot = {records committed, records dropped}.
constexpr int kOpeningKept = 12, kSideWords = 10;
constexpr int kAccWords = 2 + kOpeningKept + 2 * kSideWords;
constexpr int kRecHead = 8, kRecWords = kRecHead + kOpeningKept + 2 * kSideWords;
constexpr int kFeatCursorWords = 2;
constexpr int kSpatialMoveTypes = 139, kPromotionMin = 64, kPromotionMax = 131, kDropMin = 132, kDropMax = 138;
constexpr int kNoCapture = 255, kRookSquare = 79, kKingSquare = 76, kReasonRepetition = 2;
constexpr int kEarlyDropPly = 40, kRookMobilityPly = 20, kKingDisplacementPly = 20, kKingMovementPly = 30;

// word w of a fresh accumulator: the three optional plies of each side are -1, everything else 0
__device__ __forceinline__ int acc_reset_word(int w) {
    const int f = w - 2 - kOpeningKept;
    if (f < 0) return 0;
    const int k = f % kSideWords;
    return (k == 0 || k == 1 || k == 6) ? -1 : 0;
}

struct FeaturesArgs {
    const int* state; int E;
    const long long* actions; const uint8_t* pre_player; const int* nlegal;
    const uint8_t* captured; const uint8_t* reason; const uint16_t* ply;
    const float* rewards; const uint8_t* terminated; const uint8_t* truncated;
    int* acc; int* records; int* fcursors; int cap;
};

__global__ __launch_bounds__(kArenaThreads) void arena_features_kernel(FeaturesArgs a) {
    __shared__ int red[kArenaThreads / 64];
    __shared__ int wsum[kArenaThreads / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int e0 = s * a.E;
    const int status = a.state[kHdrWords + s * kSlotWords + 7];
    if (!(status & kSeated) || (status & kDone)) return;        // uniform over the workgroup
    int stalled = 0;
    for (int k = tid; k < a.E; k += kArenaThreads) stalled |= a.nlegal[e0 + k] == 0;
    if (ka_block_sum<kArenaThreads>(stalled, red) != 0) return; // concurrent_matches.py:303-314, :410: a skipped slot records nothing
    const int round_ply = a.state[2];
    const int first = a.fcursors[s * kFeatCursorWords + 0];
    const int room = first < 0 ? 0 : max(0, a.cap - first);     // records of this ply that still fit
    int running = 0;
    for (int base = 0; base < a.E; base += kArenaThreads) {
        const int k = base + tid;
        const bool have = k < a.E;
        const int e = e0 + (have ? k : 0);
        int* acc = a.acc + (size_t)e * kAccWords;
        bool done = false;
        int ply = 0, mover = 0;
        if (have) {                                             // game_feature_tracker.py:229-280
            const int action = (int)a.actions[e];
            ply = a.ply[e];
            mover = a.pre_player[e] & 1;
            done = a.terminated[e] || a.truncated[e];
            int* side = acc + 2 + kOpeningKept + mover * kSideWords;
            const int square = action / kSpatialMoveTypes, type = action % kSpatialMoveTypes;
            const bool drop = type >= kDropMin && type <= kDropMax;
            const int kept = acc[0];
            if (kept < kOpeningKept) {                          // :240: the first 12 actions since the reset
                acc[2 + kept] = action;
                acc[0] = kept + 1;
            }
            if (a.captured[e] != kNoCapture) {
                side[2] += 1;
                if (side[0] < 0) side[0] = ply;
            }
            if (drop) {
                side[3] += 1;
                if (side[1] < 0) side[1] = ply;
                if (ply <= kEarlyDropPly) side[5] += 1;
            }
            if (type >= kPromotionMin && type <= kPromotionMax) side[4] += 1;
            if (!drop && square == kRookSquare) {               // :264-275: 79 and 76 for both sides, board moves only
                if (side[6] < 0) side[6] = ply;
                if (ply <= kRookMobilityPly) side[7] += 1;
            }
            if (!drop && square == kKingSquare) {
                if (ply <= kKingDisplacementPly) side[8] += 1;
                if (ply <= kKingMovementPly) side[9] += 1;
            }
            if (done && a.reason[e] == kReasonRepetition) acc[1] += 1;      // :278-280
        }
        int rank;
        running += ka_tile_rank(done, running, wsum, &rank);
        if (done) {                                             // :286-356: one record per game, then a fresh accumulator
            if (rank < room) {
                int* rec = a.records + ((size_t)s * a.cap + first + rank) * kRecWords;
                const float r = a.rewards[e];
                rec[0] = e; rec[1] = ply; rec[2] = a.reason[e]; rec[3] = mover;
                rec[4] = r > 0.f ? 1 : (r < 0.f ? -1 : 0);      // :298-303 (a NaN is a draw)
                rec[5] = acc[0]; rec[6] = acc[1]; rec[7] = round_ply;
                for (int w = 2; w < kAccWords; ++w) rec[kRecHead - 2 + w] = acc[w];
            }
            for (int w = 0; w < kAccWords; ++w) acc[w] = acc_reset_word(w);
        }
    }
    if (tid == 0) {                                             // every thread has read `first` before the scan's barriers
        a.fcursors[s * kFeatCursorWords + 0] = first + min(running, room);
        a.fcursors[s * kFeatCursorWords + 1] += max(0, running - room);
    }
}

// jobs: n rows of {slot, ...} as ka_arena_assign takes them; one workgroup per job
__global__ __launch_bounds__(kArenaThreads) void arena_features_seat_kernel(const int* jobs, int slots, int E, int* acc) {
    const int s = jobs[blockIdx.x * 4];
    if (s < 0 || s >= slots) return;
    int* base = acc + (size_t)s * E * kAccWords;
    for (int i = threadIdx.x; i < E * kAccWords; i += kArenaThreads) base[i] = acc_reset_word(i % kAccWords);
}

// dynamic_trainer.py:303-318, :358: W/D/L labels of terminal rows (-1 elsewhere) and advantages = rewards x dones
__global__ void dynamic_targets_kernel(const float* rewards, const float* dones, long long* cats, float* adv, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = rewards[i], d = dones[i];
    long long c = -1;                                          // (rollout_rows.h's label gives a NaN reward 3; here it is -1)
    if (d != 0.f) c = r > 0.f ? 0 : (r == 0.f ? 1 : (r < 0.f ? 2 : -1));
    cats[i] = c;
    adv[i] = r * d;
}

}  // namespace

extern "C" int ka_arena_cursor_words(int slots) { return kCursorWords * slots; }

extern "C" int ka_arena_record_pre(const int* state, const int* side_bits, int slots, int envs_per_slot, const float* obs,
                                   const void* mask_bits, const long long* actions, const void* pre_player, const int* nlegal,
                                   int* cursors, int* row_of, float* st_obs, void* st_mask_bits, long long* st_actions,
                                   void* st_perspective, int cap, int obs_elems, int mask_words, void* stream) {
    KA_REQUIRE(state && side_bits && obs && mask_bits && actions && pre_player && nlegal && cursors && row_of && st_obs &&
               st_mask_bits && st_actions && st_perspective, "arena_record_pre: null tensor");
    KA_REQUIRE(slots > 0 && envs_per_slot > 0 && envs_per_slot <= 8192, "arena_record_pre: slots %d, envs_per_slot %d (1..8192)",
               slots, envs_per_slot);
    KA_REQUIRE(cap >= 0 && (long long)slots * cap < (1ll << 31), "arena_record_pre: cap %d x slots %d", cap, slots);
    KA_REQUIRE(obs_elems > 0 && obs_elems % 2 == 0 && mask_words > 0,
               "arena_record_pre: obs_elems %d (even: rows are copied as 8-byte vectors), mask_words %d", obs_elems, mask_words);
    KA_REQUIRE(((uintptr_t)obs | (uintptr_t)st_obs) % 8 == 0, "arena_record_pre: observation buffers must be 8-byte aligned");
    RecordPreArgs a{state, side_bits, envs_per_slot, obs, static_cast<const uint32_t*>(mask_bits), actions,
                    static_cast<const uint8_t*>(pre_player), nlegal, cursors, row_of, st_obs,
                    static_cast<uint32_t*>(st_mask_bits), st_actions, static_cast<uint8_t*>(st_perspective), cap, obs_elems,
                    mask_words};
    const int y = envs_per_slot < 64 ? envs_per_slot : 64;
    hipLaunchKernelGGL(arena_record_pre_kernel, dim3(slots, y), dim3(kArenaThreads), envs_per_slot * sizeof(int),
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("arena_record_pre");
}

extern "C" int ka_arena_record_post(int* cursors, const int* row_of, int slots, int envs_per_slot, const float* rewards,
                                    const void* terminated, const void* truncated, float* st_rewards, float* st_dones,
                                    int cap, void* stream) {
    KA_REQUIRE(cursors && row_of && rewards && terminated && truncated && st_rewards && st_dones, "arena_record_post: null tensor");
    KA_REQUIRE(slots > 0 && envs_per_slot > 0 && cap >= 0 && (long long)slots * cap < (1ll << 31),
               "arena_record_post: slots %d, envs_per_slot %d, cap %d", slots, envs_per_slot, cap);
    hipLaunchKernelGGL(arena_record_post_kernel, dim3(slots), dim3(kArenaThreads), 0, static_cast<hipStream_t>(stream), cursors,
                       row_of, envs_per_slot, rewards, static_cast<const uint8_t*>(terminated),
                       static_cast<const uint8_t*>(truncated), st_rewards, st_dones, slots * cap);
    return ka_check_launch("arena_record_post");
}

extern "C" int ka_arena_feature_words(int which) {
    return which == 0 ? kAccWords : which == 1 ? kRecWords : which == 2 ? kFeatCursorWords : -1;
}

extern "C" int ka_arena_features_step(const int* state, int slots, int envs_per_slot, const long long* actions,
                                      const void* pre_player, const int* nlegal, const void* captured, const void* reason,
                                      const void* ply, const float* rewards, const void* terminated, const void* truncated,
                                      int* acc, int* records, int* fcursors, int cap, void* stream) {
    KA_REQUIRE(state && actions && pre_player && nlegal && captured && reason && ply && rewards && terminated && truncated &&
               acc && records && fcursors, "arena_features_step: null tensor");
    KA_REQUIRE(slots > 0 && envs_per_slot > 0 && (long long)slots * envs_per_slot * kAccWords < (1ll << 31),
               "arena_features_step: slots %d, envs_per_slot %d", slots, envs_per_slot);
    KA_REQUIRE(cap >= 0 && (long long)slots * cap * kRecWords < (1ll << 31), "arena_features_step: cap %d x slots %d", cap, slots);
    KA_REQUIRE((uintptr_t)ply % 2 == 0, "arena_features_step: ply must be 2-byte aligned (uint16 payload)");
    FeaturesArgs a{state, envs_per_slot, actions, static_cast<const uint8_t*>(pre_player), nlegal,
                   static_cast<const uint8_t*>(captured), static_cast<const uint8_t*>(reason),
                   static_cast<const uint16_t*>(ply), rewards, static_cast<const uint8_t*>(terminated),
                   static_cast<const uint8_t*>(truncated), acc, records, fcursors, cap};
    hipLaunchKernelGGL(arena_features_kernel, dim3(slots), dim3(kArenaThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("arena_features_step");
}

extern "C" int ka_arena_features_seat(const int* jobs, int njobs, int slots, int envs_per_slot, int* acc, void* stream) {
    KA_REQUIRE(jobs && acc, "arena_features_seat: null tensor");
    KA_REQUIRE(njobs > 0 && slots > 0 && envs_per_slot > 0 && (long long)slots * envs_per_slot * kAccWords < (1ll << 31),
               "arena_features_seat: njobs %d, slots %d, envs_per_slot %d", njobs, slots, envs_per_slot);
    hipLaunchKernelGGL(arena_features_seat_kernel, dim3(njobs), dim3(kArenaThreads), 0, static_cast<hipStream_t>(stream), jobs,
                       slots, envs_per_slot, acc);
    return ka_check_launch("arena_features_seat");
}

extern "C" int ka_dynamic_targets(const float* rewards, const float* dones, long long* cats, float* adv, long long n, void* stream) {
    KA_REQUIRE(rewards && dones && cats && adv, "dynamic_targets: null tensor");
    KA_REQUIRE(n > 0, "dynamic_targets: n %lld", n);
    hipLaunchKernelGGL(dynamic_targets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       rewards, dones, cats, adv, n);
    return ka_check_launch("dynamic_targets");
}

extern "C" int ka_arena_state_words(int slots) { return kHdrWords + kSlotWords * slots; }

extern "C" int ka_arena_referee(int* state, int slots, int envs_per_slot, const float* rewards,
                                const void* terminated, const void* truncated, const void* players, const int* nlegal,
                                const long long* refusal, int* model_of, void* pre_player, void* stream) {
    KA_REQUIRE(state && rewards && terminated && truncated && players && nlegal && model_of && pre_player,
               "arena_referee: null tensor");
    KA_REQUIRE(slots > 0 && envs_per_slot > 0, "arena_referee: slots %d, envs_per_slot %d", slots, envs_per_slot);
    RefereeArgs a{state, envs_per_slot, rewards, static_cast<const uint8_t*>(terminated),
                  static_cast<const uint8_t*>(truncated), static_cast<const uint8_t*>(players), nlegal, refusal, model_of,
                  static_cast<uint8_t*>(pre_player)};
    hipLaunchKernelGGL(arena_referee_kernel, dim3(slots), dim3(kArenaThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("arena_referee");
}

extern "C" int ka_arena_assign(int* state, const int* jobs, int njobs, int envs_per_slot, const void* players, int* model_of,
                               void* pre_player, void* stream) {
    KA_REQUIRE(state && jobs && players && model_of && pre_player, "arena_assign: null tensor");
    KA_REQUIRE(njobs > 0 && envs_per_slot > 0, "arena_assign: njobs %d, envs_per_slot %d", njobs, envs_per_slot);
    hipLaunchKernelGGL(arena_assign_kernel, dim3(njobs), dim3(kArenaThreads), 0, static_cast<hipStream_t>(stream), state, jobs,
                       envs_per_slot, static_cast<const uint8_t*>(players), model_of, static_cast<uint8_t*>(pre_player));
    return ka_check_launch("arena_assign");
}
