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
// lies in [0, K), the row is on, its game ply (the u32 at byte 100 of its state row) is at least skip_plies and it has a
// checking move.
//
// Record of an env, 4 + cap int32 words:
//   0 flags (bit 0 active, bit 1 mate found, bit 2 the action was changed, bit 3 truncated: more checking moves than forked)
//   1 checking moves, uncapped (0 for an env the controls leave out: they are not counted)   2 slot of the mate played, -1
//   3 action played (the incoming action unless bit 2)   4.. the checking actions forked, ascending, -1 = unused
//
// The fork is one workgroup per env and walks the set bits of the mask row, never the action space.  The checking moves
// are compacted in ascending action order across the whole workgroup: a block scan over the per-thread counts of each pass
// of 256 mask words.  The copies are those of the lookahead's fork (csrc/lookahead.hip), 16 bytes per lane where the rows
// allow it.  Unused and inactive slots get the state, the mask and the env's own incoming action (legal whenever the main
// step's is: one refused action makes the env step hold every row of its launch); their history is not copied and nothing
// reads their outcome.  The parent's rows are only read.  Kernel nodes only, caller-owned buffers, no workgroup waits for
// another.
#include "common.h"

#include <climits>

namespace {

constexpr int kMtThreads = 256, kMtWaves = kMtThreads / 64;
constexpr int kMtSlots = 139, kMtA = 81 * kMtSlots, kMtMaxCap = 64;
constexpr int kMtWords = (kMtA + 31) / 32;
constexpr uint32_t kMtTailBits = (1u << (kMtA - 32 * (kMtWords - 1))) - 1u;       // the bits of the last word that are actions
constexpr int kMtStateBytes = 128, kMtSideByte = 95, kMtPlyByte = 100;            // csrc/shogi_env.hip, kStateBytes
constexpr int kMtFlags = 0, kMtNChecks = 1, kMtSlot = 2, kMtAction = 3, kMtList = 4;
constexpr int kMtTableWords = 4, kMtStatsWords = 5;                               // (the error word follows the stats)
constexpr int kMtStateUnits = kMtStateBytes / 16, kMtMaskUnits = kMtWords * 4 / 16;     // 16-byte pieces of a state / mask row
static_assert(kMtWords * 4 % 16 == 0 && kMtStateBytes % 16 == 0, "state and mask rows are copied in 16-byte pieces");
constexpr int R_CHECKMATE = 1;                                                    // step_result.rs:9-16

__host__ __device__ constexpr int mt_words(int cap) { return kMtList + cap; }

// ---- the few rule helpers of csrc/shogi_env.hip, restated: that file stays as it is
enum { PAWN = 1, LANCE, KNIGHT, SILVER, GOLD, BISHOP, ROOK, KING };
constexpr int WHITE_BIT = 0x10, PROM_BIT = 0x20;

// directions: N NE E SE S SW W NW; "N" is toward row 0
__device__ __forceinline__ int dir_dr(int d) { return ((0x1A90 >> (2 * d)) & 3) - 1; }      // -1 -1 0 1 1 1 0 -1
__device__ __forceinline__ int dir_dc(int d) { return ((0x01A9 >> (2 * d)) & 3) - 1; }      //  0  1 1 1 0 -1 -1 -1

// step (low byte) and slide (high byte) direction sets of every piece byte, in board directions
__host__ __device__ constexpr unsigned dirs_of(int pc) {
    const unsigned N = 1, NE = 2, E = 4, SE = 8, S = 16, SW = 32, W = 64, NW = 128, gold = N | NE | NW | E | W | S;
    const int t = pc & 15;
    const bool pr = pc & PROM_BIT, wh = pc & WHITE_BIT;
    unsigned st = 0, sl = 0;
    if (pr) {
        if (t == PAWN || t == LANCE || t == KNIGHT || t == SILVER) st = gold;
        else if (t == BISHOP) { st = N | E | S | W; sl = NE | SE | SW | NW; }
        else if (t == ROOK) { st = NE | SE | SW | NW; sl = N | E | S | W; }
    } else {
        if (t == PAWN) st = N;
        else if (t == LANCE) sl = N;
        else if (t == SILVER) st = N | NE | NW | SE | SW;
        else if (t == GOLD) st = gold;
        else if (t == BISHOP) sl = NE | SE | SW | NW;
        else if (t == ROOK) sl = N | E | S | W;
        else if (t == KING) st = 255;
    }
    if (wh) { st = ((st << 4) | (st >> 4)) & 255; sl = ((sl << 4) | (sl >> 4)) & 255; }
    return st | (sl << 8);
}

// the board in LDS with up to two squares replaced
typedef const __attribute__((address_space(3))) uint8_t* lds_board;
typedef const __attribute__((address_space(3))) uint16_t* lds_dirs;      // dirs_of() of every piece byte, in LDS
struct View { lds_board b; lds_dirs dirs; int o1, p1, o2, p2; };
__device__ __forceinline__ int at(const View& v, int sq) { return sq == v.o1 ? v.p1 : sq == v.o2 ? v.p2 : v.b[sq]; }

// is `sq` attacked by a piece of colour `by`?  Looks outward from the square: the first piece met along each of the
// eight lines attacks it if it steps (distance 1) or slides back along that line; plus the two knight origins.
// One probe = one line (d < 8) or one knight origin (d = 8, 9).
__device__ __forceinline__ bool attacked_from(const View& v, int sq, int by, int d) {
    const int r = sq / 9, c = sq % 9;
    if (d < 8) {
        const int dr = dir_dr(d), dc = dir_dc(d);
        const unsigned need = 1u << ((d + 4) & 7);
        int rr = r + dr, cc = c + dc, k = 1;
        while ((unsigned)rr < 9u && (unsigned)cc < 9u) {
            const int p = at(v, rr * 9 + cc);
            if (p) {
                if (((p >> 4) & 1) != by) return false;
                const unsigned m = v.dirs[p & 63];
                return (k == 1 && (m & need)) || ((m >> 8) & need);
            }
            rr += dr; cc += dc; ++k;
        }
        return false;
    }
    const int kr = by ? r - 2 : r + 2, kc = c + (d == 8 ? -1 : 1);
    return (unsigned)kr < 9u && (unsigned)kc < 9u && at(v, kr * 9 + kc) == (KNIGHT | (by ? WHITE_BIT : 0));
}

// does legal action j of `side` leave the king on `king` attacked?  The decoding of csrc/shogi_env.hip's step: slots
// 0..127 ray moves with the promote bit, 128..131 knight jumps, 132..138 drops, all in the mover's perspective.  A set bit
// that is no move on the board (a mask row the env did not write) gives no check.
__device__ bool mt_gives_check(lds_board b, lds_dirs dirs, int j, int side, int king) {
    const int sq_p = j / kMtSlots, slot = j - sq_p * kMtSlots;
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
    const uint32_t* lw = a.legal + (size_t)e * kMtWords;
    const uint8_t* st = a.state + (size_t)e * kMtStateBytes;
    const uint32_t ply = *reinterpret_cast<const uint32_t*>(st + kMtPlyByte);
    const int side = st[kMtSideByte] & 1;
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
        for (int w0 = 0; w0 < kMtWords; w0 += kMtThreads) {
            const int w = w0 + tid;
            uint32_t chk = 0u;
            if (w < kMtWords && king >= 0) {
                uint32_t m = w == kMtWords - 1 ? lw[w] & kMtTailBits : lw[w];     // (bits past the action space are dropped)
                while (m) {
                    const int bit = __builtin_ctz(m);
                    if (mt_gives_check(brd, drs, (w << 5) + bit, side, king)) chk |= 1u << bit;
                    m &= m - 1u;
                }
            }
            const int cnt = __popc(chk);
            int inc = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o);
                if (lane >= o) inc += t;
            }
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
        if (tid == kMtFlags) word = (n_fork > 0 ? 1u : 0u) | (n_checks > n_fork ? 8u : 0u);
        else if (tid == kMtNChecks) word = (uint32_t)n_checks;
        else if (tid == kMtSlot) word = (uint32_t)-1;
        else if (tid == kMtAction) word = (uint32_t)(int)(incoming < -1 ? -1 : incoming > kMtA ? kMtA : incoming);
        else word = (uint32_t)(tid - kMtList < n_fork ? s_list[tid - kMtList] : -1);
        a.rec[(size_t)e * W + tid] = word;
    }

    // ---- the child rows e * cap + j: state and mask for every slot, the history for the slots in use
    {
        const uint4* s_src = reinterpret_cast<const uint4*>(st);
        const uint4* m_src = reinterpret_cast<const uint4*>(lw);
        constexpr int kUnits = kMtStateUnits + kMtMaskUnits;
        for (int u = tid; u < kUnits * cap; u += kMtThreads) {
            const int j = u / kUnits, r = u % kUnits;
            const size_t c = (size_t)e * cap + j;
            if (r < kMtStateUnits) reinterpret_cast<uint4*>(a.c_state + c * kMtStateBytes)[r] = s_src[r];
            else reinterpret_cast<uint4*>(a.c_bits + c * kMtWords)[r - kMtStateUnits] = m_src[r - kMtStateUnits];
        }
    }
    const int hist = a.hist, n = (int)min(ply, (uint32_t)hist);            // entries [0, ply) of the env's history rows
    if (n_fork > 0 && n > 0) {
        const unsigned long long* k_src = a.keys + (size_t)e * hist;
        if ((hist & 1) == 0) {                                 // rows of an even number of keys start at 16-byte boundaries
            const int units = (n + 1) >> 1;                    // (an odd count takes one stale key along: it stays inside the row)
            for (int u = tid; u < units * n_fork; u += kMtThreads) {
                const int j = u / units, r = u % units;
                reinterpret_cast<uint4*>(a.c_keys + ((size_t)e * cap + j) * hist)[r] = reinterpret_cast<const uint4*>(k_src)[r];
            }
        } else {
            for (int u = tid; u < n * n_fork; u += kMtThreads) {
                const int j = u / n, r = u % n;
                a.c_keys[((size_t)e * cap + j) * hist + r] = k_src[r];
            }
        }
        const uint8_t* c_src = a.checks + (size_t)e * hist;
        if ((hist & 15) == 0) {
            const int units = (n + 15) >> 4;
            for (int u = tid; u < units * n_fork; u += kMtThreads) {
                const int j = u / units, r = u % units;
                reinterpret_cast<uint4*>(a.c_checks + ((size_t)e * cap + j) * hist)[r] = reinterpret_cast<const uint4*>(c_src)[r];
            }
        } else if ((hist & 3) == 0) {
            const int units = (n + 3) >> 2;
            for (int u = tid; u < units * n_fork; u += kMtThreads) {
                const int j = u / units, r = u % units;
                reinterpret_cast<uint32_t*>(a.c_checks + ((size_t)e * cap + j) * hist)[r] = reinterpret_cast<const uint32_t*>(c_src)[r];
            }
        } else {
            for (int u = tid; u < n * n_fork; u += kMtThreads) {
                const int j = u / n, r = u % n;
                a.c_checks[((size_t)e * cap + j) * hist + r] = c_src[r];
            }
        }
    }
    if (tid < cap) a.c_actions[(size_t)e * cap + tid] = tid < n_fork ? (long long)s_list[tid] : incoming;
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
        if (flags & 1u) {
            active = true;
            truncated = (flags & 8u) != 0;
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
                rec[kMtFlags] = flags | 2u | (changed ? 4u : 0u);
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
    KA_REQUIRE(A == kMtA, "mate_fork: the spatial action space only (A = %d), got %d", kMtA, A);
    KA_REQUIRE(legal_words == kMtWords, "mate_fork: packed mask rows of %d words", kMtWords);
    KA_REQUIRE(cap >= 1 && cap <= kMtMaxCap, "mate_fork: cap must lie in [1, %d], got %d", kMtMaxCap, cap);
    KA_REQUIRE(K >= 1, "mate_fork: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE(max_ply >= 0 && max_ply <= 65535, "mate_fork: max_ply must lie in [0, 65535], got %d", max_ply);
    KA_REQUIRE((long long)N * cap <= INT_MAX, "mate_fork: %d envs of cap %d are too many child rows", N, cap);
    KA_REQUIRE((uintptr_t)table % 4 == 0, "mate_fork: the controls table is aligned to its 32-bit words");
    KA_REQUIRE((uintptr_t)legal % 16 == 0 && (uintptr_t)actions % 8 == 0 && (uintptr_t)model_of % 4 == 0 &&
               (uintptr_t)records % 4 == 0 && (uintptr_t)state % 16 == 0 && (uintptr_t)keys % 16 == 0 &&
               (uintptr_t)checks % 16 == 0 && (uintptr_t)child_state % 16 == 0 && (uintptr_t)child_keys % 16 == 0 &&
               (uintptr_t)child_checks % 16 == 0 && (uintptr_t)child_mask_bits % 16 == 0 && (uintptr_t)child_actions % 8 == 0,
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
    KA_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)child_rewards % 4 == 0 && (uintptr_t)child_err % 8 == 0 &&
               (uintptr_t)actions % 8 == 0 && (uintptr_t)stats % 4 == 0 && (uintptr_t)err % 4 == 0,
               "mate_choose: actions and the child error words are 8-byte aligned, every other tensor to its element size");
    MateChooseArgs a{static_cast<uint32_t*>(records), cap, child_rewards, static_cast<const uint8_t*>(child_terminated),
                     static_cast<const uint8_t*>(child_reason), static_cast<const unsigned long long*>(child_err), actions, stats,
                     err, N};
    hipLaunchKernelGGL(mate_choose_kernel, dim3((N + kMtThreads - 1) / kMtThreads), dim3(kMtThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mate_choose");
}
