// Mate in one in the device ply.  The sampler, the lookahead and the tree search all judge a move through the value head;
// none asks the rules the one question a shogi program answers exactly: can the side to move mate now?  A game is a few
// rows of device memory and ka_shogi_env_step already decides checkmate exactly, so the answer is "find the moves worth
// trying, copy rows, step them with the env kernel as it is, look at the verdicts":
//
//   ka_mate_fork            per env: the legal moves that give check, in ascending action order; the first `cap` of them
//                           become child rows: state, history, mask, action
//   ka_shogi_env_step       (csrc/shogi_env.hip, unchanged) over the N * cap child rows
//   ka_mate_choose          per env: a child that ended by checkmate in the mover's favour replaces actions[e]
//
// Only a checking move can mate, and finding the checking moves needs no move generation: the legal moves are the set bits
// of the env's packed mask row.  Each is decoded in the mover's perspective (csrc/shogi_env.hip, the decoding of the step),
// laid over the board in LDS -- a board move is two overlay squares (from empty, to the piece or its promoted byte; a
// capture falls out of the overlay), a drop is one -- and the other king is tested by looking outward from it, which
// catches direct, discovered and double checks alike.  Whether the check is a mate is the env step's verdict and nothing
// else: a checking move that ends the game by repetition, perpetual check or the move limit is not a mate.
//
// Row m of the controls table (device memory, read by every launch: a new table applies from the next ply of a captured
// graph) belongs to model m:   word 0 int32 max_checks (0 = off, 1..64)   1 int32 skip_plies (>= 0)   2, 3 reserved, zero
// A row outside these ranges reads as off; max_checks above the launch's cap is cut to it.  An env is active when its model
// lies in [0, K), the row is on, its game ply (the ply word of its state row) is at least skip_plies and it has a checking
// move.
//
// Record of an env, 4 + cap int32 words (csrc/mate_record.h names them):
//   0 flags (bit 0 active, bit 1 mate found, bit 2 the action was changed, bit 3 truncated: more checking moves than forked)
//   1 checking moves, uncapped (0 for an env the controls leave out: they are not counted)   2 slot of the mate played, -1
//   3 action played (the incoming action unless bit 2)   4.. the checking actions forked, ascending, -1 = unused
//
// The fork is one workgroup per env and walks the set bits of the mask row, never the action space.  The checking moves
// are compacted in ascending action order across the whole workgroup: a block scan over the per-thread counts of each pass
// of 256 mask words.  The rule helpers are the env's (csrc/shogi_rules.h) and the copy is the ply's one fork copy
// (csrc/ply_rows.h).  Unused and inactive slots get the state, the mask and the env's own incoming action (legal whenever
// the main step's is: one refused action makes the env step hold every row of its launch); their history is not copied and
// nothing reads their outcome.  The parent's rows are only read.  Kernel nodes only, caller-owned buffers, no workgroup
// waits for another.
#include "mate_record.h"
#include "ply_rows.h"

#include <climits>

namespace {

constexpr int kMtThreads = 256, kMtWaves = kMtThreads / 64;
constexpr int kMtMaxCap = 64;
constexpr int kMtTableWords = 4, kMtStatsWords = 5;                               // (the error word follows the stats)

// does legal action j of `side` leave the king on `king` attacked?  The decoding of csrc/shogi_env.hip's step: slots
// 0..127 ray moves with the promote bit, 128..131 knight jumps, 132..138 drops, all in the mover's perspective.  A set bit
// that is no move on the board (a mask row the env did not write) gives no check.
__device__ bool mt_gives_check(lds_board b, lds_dirs dirs, int j, int side, int king) {
    const int sq_p = j / kPlySlots, slot = j - sq_p * kPlySlots;
    const int fr = sq_p / 9, fc = sq_p % 9;
    int tr = fr, tc = fc, promote = 0, drop = -1;
    if (slot < 128) {
        promote = slot >= 64;
        const int s = slot & 63, d = s >> 3, dist = (s & 7) + 1;
        tr = fr + dir_dr(d) * dist; tc = fc + dir_dc(d) * dist;
    } else if (slot < 132) {
        const int k = slot - 128;
        promote = k & 1; tr = fr - 2; tc = fc + ((k >> 1) ? 1 : -1);
    } else {
        drop = slot - 132;
    }
    if ((unsigned)tr >= 9u || (unsigned)tc >= 9u) return false;
    const int to_p = tr * 9 + tc, to = side ? 80 - to_p : to_p;
    View v{b, dirs, to, (drop + 1) | (side ? WHITE_BIT : 0), -1, 0};
    if (drop < 0) {
        const int from = side ? 80 - sq_p : sq_p, pc = b[from];
        v = View{b, dirs, from, 0, to, promote ? pc | PROM_BIT : pc};
    }
#pragma unroll 1
    for (int d = 0; d < 10; ++d) if (attacked_from(v, king, side, d)) return true;
    return false;
}

// the controls of model m as the kernels read them: max_checks (0 = off) and skip_plies
__device__ __forceinline__ int mt_controls(const uint32_t* table, int m, int K, int* skip) {
    *skip = 0;
    if (m < 0 || m >= K) return 0;
    const uint32_t* c = table + (size_t)m * kMtTableWords;
    const int mc = (int)c[0], s = (int)c[1];
    if (!(mc >= 0 && mc <= kMtMaxCap && s >= 0)) return 0;
    *skip = s;
    return mc;
}

struct MateForkArgs {
    const uint32_t* legal; const long long* actions; const int* model_of; int K; const uint32_t* table;
    const uint8_t* state; const unsigned long long* keys; const uint8_t* checks; int hist; int cap;
    uint32_t* rec; uint8_t* c_state; unsigned long long* c_keys; uint8_t* c_checks; uint32_t* c_bits; long long* c_actions;
};

struct MateChooseArgs {
    uint32_t* rec; int cap; const float* rewards; const uint8_t* term; const uint8_t* reason;
    const unsigned long long* c_err; long long* actions; int* stats; int* err; int n;
};

__global__ __launch_bounds__(kMtThreads) void mate_fork_kernel(MateForkArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_board[96];
    __shared__ uint16_t s_dirs[64];
    __shared__ int s_king;
    __shared__ int s_wave[kMtWaves];
    __shared__ int s_list[kMtMaxCap];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = a.cap, W = mt_words(cap);
    const uint32_t* lw = a.legal + (size_t)e * kPlyWords;
    const uint8_t* st = a.state + (size_t)e * kStateBytes;
    const uint32_t ply = *reinterpret_cast<const uint32_t*>(st + kPlyByte);
    const int side = st[kSideByte] & 1;
    int skip;
    int want = min(mt_controls(a.table, a.model_of[e], a.K, &skip), cap);       // (uniform over the workgroup, as every branch below)
    if (ply < (uint32_t)skip) want = 0;

    int n_checks = 0;
    if (want > 0) {
        if (tid < 81) s_board[tid] = st[tid];
        if (tid < 64) s_dirs[tid] = (uint16_t)dirs_of(tid);
        if (tid == 0) s_king = -1;
        __syncthreads();
        if (tid < 81 && s_board[tid] == (KING | (side ? 0 : WHITE_BIT))) s_king = tid;      // the other king
        __syncthreads();
        const int king = s_king;
        const lds_board brd = (lds_board)s_board;
        const lds_dirs drs = (lds_dirs)s_dirs;
        // a pass = 256 consecutive mask words, one per thread: thread order is action order, so an exclusive block scan of
        // the counts places every thread's checking moves
        for (int w0 = 0; w0 < kPlyWords; w0 += kMtThreads) {
            const int w = w0 + tid;
            uint32_t chk = 0u;
            if (w < kPlyWords && king >= 0) {
                uint32_t m = mask_word(lw, w);
                while (m) {
                    const int bit = __builtin_ctz(m);
                    if (mt_gives_check(brd, drs, (w << 5) + bit, side, king)) chk |= 1u << bit;
                    m &= m - 1u;
                }
            }
            const int cnt = __popc(chk), inc = ka_wave_scan(cnt);
            __syncthreads();                                   // (the pass before has read s_wave)
            if (lane == 63) s_wave[wave] = inc;
            __syncthreads();
            int pos = n_checks + inc - cnt, total = 0;
            for (int x = 0; x < kMtWaves; ++x) {
                if (x < wave) pos += s_wave[x];
                total += s_wave[x];
            }
            while (chk && pos < kMtMaxCap) {
                s_list[pos++] = (w << 5) + __builtin_ctz(chk);
                chk &= chk - 1u;
            }
            n_checks += total;
        }
        __syncthreads();                                       // s_list
    }
    const int n_fork = min(n_checks, want);                    // > 0: the env is active
    const long long incoming = a.actions[e];

    if (tid < W) {
        uint32_t word = 0u;
        if (tid == kMtFlags) word = (n_fork > 0 ? kMtActive : 0u) | (n_checks > n_fork ? kMtTruncated : 0u);
        else if (tid == kMtNChecks) word = (uint32_t)n_checks;
        else if (tid == kMtSlot) word = (uint32_t)-1;
        else if (tid == kMtAction) word = (uint32_t)(int)(incoming < -1 ? -1 : incoming > kPlyA ? kPlyA : incoming);
        else word = (uint32_t)(tid - kMtList < n_fork ? s_list[tid - kMtList] : -1);
        a.rec[(size_t)e * W + tid] = word;
    }

    // ---- the child rows e * cap + j: the env's state and mask for every slot, entries [0, ply) of its history for the
    // slots in use
    const int hist = a.hist;
    const size_t c0 = (size_t)e * cap;
    const PlyRow parent{st, lw, a.keys + (size_t)e * hist, a.checks + (size_t)e * hist};
    ply_fork_rows<kMtThreads>(PlyRows{a.c_state + c0 * kStateBytes, a.c_bits + c0 * kPlyWords, a.c_keys + c0 * hist,
                                      a.c_checks + c0 * hist},
                              cap, n_fork, hist, (int)min(ply, (uint32_t)hist), [&](int) { return parent; });
    if (tid < cap) a.c_actions[c0 + tid] = tid < n_fork ? (long long)s_list[tid] : incoming;
}

// one thread per env: at most 64 children each
__global__ __launch_bounds__(kMtThreads) void mate_choose_kernel(MateChooseArgs a) {
    const int e = blockIdx.x * kMtThreads + threadIdx.x, lane = threadIdx.x & 63;
    const int cap = a.cap, W = mt_words(cap);
    // a refused child step moved no child: its outputs are the unchanged positions, so nothing is chosen from them
    const bool held = a.c_err && (a.c_err[0] | a.c_err[1]) != 0ull;
    bool active = false, mate = false, changed = false, truncated = false;
    int forked = 0;
    if (e < a.n && !held) {
        uint32_t* rec = a.rec + (size_t)e * W;
        const uint32_t flags = rec[kMtFlags];
        if (flags & kMtActive) {
            active = true;
            truncated = (flags & kMtTruncated) != 0;
            const long long incoming = a.actions[e];
            int first = -1, keep = -1;
            for (int j = 0; j < cap; ++j) {
                const int act = (int)rec[kMtList + j];
                if (act < 0) break;                            // the slots in use come first
                ++forked;
                const size_t c = (size_t)e * cap + j;
                if (a.term[c] && a.reason[c] == R_CHECKMATE && a.rewards[c] > 0.f) {
                    if (first < 0) first = j;                  // (ascending actions: the lowest)
                    if ((long long)act == incoming) keep = j;
                }
            }
            if (first >= 0) {
                const int slot = keep >= 0 ? keep : first, act = (int)rec[kMtList + slot];
                mate = true;
                changed = keep < 0;
                rec[kMtSlot] = (uint32_t)slot;
                rec[kMtAction] = (uint32_t)act;
                rec[kMtFlags] = flags | kMtMate | (changed ? kMtChanged : 0u);
                if (changed) a.actions[e] = act;
            }
        }
    }
    const int na = __popcll(__ballot(active)), nm = __popcll(__ballot(mate)), nc = __popcll(__ballot(changed));
    const int nt = __popcll(__ballot(truncated));
    int nf = forked;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o);
    if (lane == 0) {
        if (na) atomicAdd(&a.stats[0], na);
        if (nf) atomicAdd(&a.stats[1], nf);
        if (nm) atomicAdd(&a.stats[2], nm);
        if (nc) atomicAdd(&a.stats[3], nc);
        if (nt) atomicAdd(&a.stats[4], nt);
        if (held && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.err[0], 2);
    }
}

}  // namespace

extern "C" int ka_mate_words(int which, int cap) {
    if (cap < 0 || cap > kMtMaxCap) return -1;
    return which == 0 ? mt_words(cap) : which == 1 ? kMtTableWords : which == 2 ? kMtStatsWords + 1 : which == 3 ? kMtMaxCap : -1;
}

extern "C" int ka_mate_fork(const void* legal, int legal_words, const long long* actions, const int* model_of, int K,
                            const void* table, const void* state, const void* keys, const void* checks, int max_ply, int cap,
                            void* records, void* child_state, void* child_keys, void* child_checks, void* child_mask_bits,
                            long long* child_actions, int N, int A, void* stream) {
    KA_REQUIRE(legal && actions && model_of && table && state && keys && checks && records && child_state && child_keys &&
               child_checks && child_mask_bits && child_actions && N > 0, "mate_fork: null tensor");
    KA_REQUIRE_PLY_SPACE("mate_fork", A, legal_words);
    KA_REQUIRE(cap >= 1 && cap <= kMtMaxCap, "mate_fork: cap must lie in [1, %d], got %d", kMtMaxCap, cap);
    KA_REQUIRE(K >= 1, "mate_fork: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE_MAX_PLY("mate_fork", max_ply);
    KA_REQUIRE((long long)N * cap <= INT_MAX, "mate_fork: %d envs of cap %d are too many child rows", N, cap);
    KA_REQUIRE((uintptr_t)table % 4 == 0, "mate_fork: the controls table is aligned to its 32-bit words");
    KA_REQUIRE(ka_aligned(16, {legal, state, keys, checks, child_state, child_keys, child_checks, child_mask_bits}) &&
               ka_aligned(8, {actions, child_actions}) && ka_aligned(4, {model_of, records}),
               "mate_fork: state, history and mask rows are 16-byte aligned, every other tensor to its element size");
    MateForkArgs a{static_cast<const uint32_t*>(legal), actions, model_of, K, static_cast<const uint32_t*>(table),
                   static_cast<const uint8_t*>(state), static_cast<const unsigned long long*>(keys),
                   static_cast<const uint8_t*>(checks), max_ply > 0 ? max_ply : 1, cap, static_cast<uint32_t*>(records),
                   static_cast<uint8_t*>(child_state), static_cast<unsigned long long*>(child_keys),
                   static_cast<uint8_t*>(child_checks), static_cast<uint32_t*>(child_mask_bits), child_actions};
    hipLaunchKernelGGL(mate_fork_kernel, dim3(N), dim3(kMtThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mate_fork");
}

extern "C" int ka_mate_choose(void* records, int cap, const float* child_rewards, const void* child_terminated,
                              const void* child_reason, const void* child_err, long long* actions, int* stats, int* err, int N,
                              void* stream) {
    KA_REQUIRE(records && child_rewards && child_terminated && child_reason && actions && stats && err && N > 0,
               "mate_choose: null tensor");
    KA_REQUIRE(cap >= 1 && cap <= kMtMaxCap, "mate_choose: cap must lie in [1, %d], got %d", kMtMaxCap, cap);
    KA_REQUIRE((long long)N * cap <= INT_MAX, "mate_choose: %d envs of cap %d are too many child rows", N, cap);
    KA_REQUIRE(ka_aligned(8, {child_err, actions}) && ka_aligned(4, {records, child_rewards, stats, err}),
               "mate_choose: actions and the child error words are 8-byte aligned, every other tensor to its element size");
    MateChooseArgs a{static_cast<uint32_t*>(records), cap, child_rewards, static_cast<const uint8_t*>(child_terminated),
                     static_cast<const uint8_t*>(child_reason), static_cast<const unsigned long long*>(child_err), actions, stats,
                     err, N};
    hipLaunchKernelGGL(mate_choose_kernel, dim3((N + kMtThreads - 1) / kMtThreads), dim3(kMtThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mate_choose");
}
