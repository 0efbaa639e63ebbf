// Mate in three in the device ply, behind the mate in one of csrc/mate.hip.  The root's checking moves are already forked
// and stepped there; what a mate in three adds is the middle ply -- the defender's replies to every check and the AND over
// them -- and a mate in one at every reply's position, which is csrc/mate.hip again with the grandchild rows as its envs:
//
//   ka_mate_fork, ka_shogi_env_step, ka_mate_choose      (unchanged) the root: checks c_0 .. c_{k-1}, their child rows
//   ka_mate3_fork           per env: the budget walk over the children, then one grandchild row per evasion of every child
//                           that gets rows: state, history, mask, action
//   ka_shogi_env_step       (unchanged) over the N * G grandchild rows
//   ka_mate3_gate           per grandchild row: the model index the third ply runs it under (-1 = not at all) and a legal
//                           filler action for that fork's unused slots
//   ka_mate_fork, ka_shogi_env_step, ka_mate_choose      (unchanged) the third ply: N * G "envs" of cap3 rows each, a
//                           second K x 4 table (word 0 reply_checks, word 1 zero), a scratch action array
//   ka_mate3_choose         per env: the proving set, the choice, the record, the counters
//
// Words 2 and 3 of the controls row of model m (csrc/mate.hip reads words 0 and 1 only):
//   2 int32 evasion_rows (0 = mate in one only, 1..128)   3 int32 reply_checks (0..64)
// A row whose words 2 / 3 lie outside these ranges has depth three off; its mate in one is what words 0 / 1 say.
//
// Env e is active at depth three when its mate-in-one record has bit 0 (active) set and bit 1 (mate) clear and
// evasion_rows > 0.  Child i (root slot i) is open when its step neither terminated nor truncated it; n_i is the number of
// set bits of its new mask: the defender is in check, so these are the evasions.  The budget walk goes over the slots in
// order with left = min(evasion_rows, G): an open child with 1 <= n_i <= left gets the next n_i of the env's G grandchild
// rows, one per evasion in ascending action order, and left -= n_i; an open child with n_i > left is skipped (flag bit 3)
// and the walk goes on.  A grandchild that its step terminated or truncated refutes its check whatever ended it and
// whatever the restarted row then shows.  Child i proves when it got rows and every grandchild of it is open and has a mate
// in one among the checks the third ply forked for it.  An incoming action that proves stays; otherwise the proving check
// with the lowest action replaces actions[e].  A cap or a budget that cuts something yields "not proven", never a mate.
//
// Record of an env, 6 + 2 * cap int32 words (cap: the root's child rows per env):
//   0 flags: bit 0 active at depth three, 1 mate in three found, 2 the action was changed, 3 a child was skipped by the
//     budget, 4 a refuting (open, mateless) grandchild's third-ply fork was truncated
//   1 grandchild rows used   2 slot played, -1   3 action played (the incoming action unless bit 2)
//   4, 5 the proving set, a 64-bit mask over the slots (low word first)
//   6 .. 6 + cap          n_i of slot i, -1 for a slot that is unused or not open
//   6 + cap .. 6 + 2 cap  the first grandchild row (0 .. G - 1 within the env) of slot i, -1 without rows
// Counters: 0 positions active at depth three, 1 grandchild rows used, 2 third-ply rows used, 3 mates in three, 4 actions
// changed, 5 children skipped; the error word follows (bit 1 the root's child step refused an action, bit 2 the grandchild
// step, bit 3 the third ply's: nothing is replaced then).
//
// The fork is one workgroup per env.  One wave owns one child at a time: its lanes count the child's mask row, and -- after
// one thread has walked the budget -- take six consecutive mask words each, so a wave scan of the lanes' counts places every
// evasion in ascending action order; a child's rows are written by one wave alone, so no order is lost between waves.  The
// copies then run over the whole workgroup: the ply's one fork copy (csrc/ply_rows.h).  Unused rows get the root env's
// state, mask and incoming action (legal whenever the main step's is: one refused action makes the env step hold every
// row of its launch); their history is not copied and nothing reads their outcome.  Kernel nodes only, caller-owned
// buffers, no workgroup waits for another.
#include "mate_record.h"
#include "ply_rows.h"

#include <climits>

namespace {

constexpr int kM3Threads = 256, kM3Waves = kM3Threads / 64;
constexpr int kM3MaxCap = 64, kM3MaxRows = 128;
constexpr int kM3LaneWords = (kPlyWords + 63) / 64;                               // consecutive mask words of one lane
constexpr int kM3TableWords = 4, kM3StatsWords = 6;                               // (the error word follows the stats)
// this file's record (the root's and the third ply's are csrc/mate_record.h's)
constexpr int kM3Flags = 0, kM3Rows = 1, kM3Slot = 2, kM3Action = 3, kM3Proving = 4, kM3N = 6;
constexpr uint32_t kM3Active = 1u, kM3Mate = 2u, kM3Changed = 4u, kM3Skipped = 8u, kM3Cut3 = 16u;

__host__ __device__ constexpr int m3_words(int cap) { return kM3N + 2 * cap; }

// evasion_rows of model m as the kernels read it (0 = depth three off)
__device__ __forceinline__ int m3_controls(const uint32_t* table, int m, int K) {
    if (m < 0 || m >= K) return 0;
    const uint32_t* c = table + (size_t)m * kM3TableWords;
    const int er = (int)c[2], rc = (int)c[3];
    if (!(er >= 0 && er <= kM3MaxRows && rc >= 0 && rc <= kM3MaxCap)) return 0;
    return er;
}

struct Mate3ForkArgs {
    const uint32_t* legal; const long long* actions; const int* model_of; int K; const uint32_t* table;
    const uint8_t* state; const uint32_t* rec1; int cap;
    const uint8_t* c_state; const unsigned long long* c_keys; const uint8_t* c_checks; const uint32_t* c_bits;
    const uint8_t* c_term; const uint8_t* c_trunc; int hist; int G;
    uint32_t* rec; uint8_t* g_state; unsigned long long* g_keys; uint8_t* g_checks; uint32_t* g_bits; long long* g_actions;
};

struct Mate3GateArgs {
    const uint32_t* rec; int cap; int G; const int* model_of; const uint32_t* g_bits; const uint8_t* g_term;
    const uint8_t* g_trunc; int* g_model; long long* g_filler; int rows;
};

struct Mate3ChooseArgs {
    uint32_t* rec; const uint32_t* rec1; int cap; int G; const uint32_t* rec3; int cap3; const uint8_t* g_term;
    const uint8_t* g_trunc; const int* model_of; int K; const uint32_t* table3; const unsigned long long* err1;
    const unsigned long long* err2; const unsigned long long* err3; long long* actions; int* stats; int* err; int n;
};

__global__ __launch_bounds__(kM3Threads) void mate3_fork_kernel(Mate3ForkArgs a) {
    __shared__ int s_n[kM3MaxCap], s_first[kM3MaxCap];
    __shared__ int s_act[kM3MaxRows], s_src[kM3MaxRows];
    __shared__ int s_used, s_skipped;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = a.cap, G = a.G, W1 = mt_words(cap), W = m3_words(cap);
    const uint32_t* rec1 = a.rec1 + (size_t)e * W1;
    const uint32_t* lw = a.legal + (size_t)e * kPlyWords;
    const uint8_t* st = a.state + (size_t)e * kStateBytes;
    const uint32_t flags1 = rec1[kMtFlags];
    const int rows = min(m3_controls(a.table, a.model_of[e], a.K), G);
    const bool active = (flags1 & kMtActive) && !(flags1 & kMtMate) && rows > 0;       // (uniform over the workgroup, as every branch below)

    if (tid < kM3MaxCap) { s_n[tid] = -1; s_first[tid] = -1; }
    if (tid < kM3MaxRows) { s_act[tid] = 0; s_src[tid] = 0; }  // (no row ever names a child outside the env's own)
    if (tid == 0) { s_used = 0; s_skipped = 0; }
    __syncthreads();
    if (active) {
        // n_i of the open children: one wave per child, the mask row read 64 words at a time
        for (int j = wave; j < cap; j += kM3Waves) {
            if ((int)rec1[kMtList + j] < 0) break;             // the slots in use come first
            const size_t c = (size_t)e * cap + j;
            if (a.c_term[c] | a.c_trunc[c]) continue;
            const uint32_t* row = a.c_bits + c * kPlyWords;
            int cnt = 0;
            for (int w = lane; w < kPlyWords; w += 64) cnt += __popc(mask_word(row, w));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
            if (lane == 0) s_n[j] = cnt;
        }
        __syncthreads();
        if (tid == 0) {                                        // the budget walk, in slot order
            int left = rows, used = 0, skipped = 0;
            for (int j = 0; j < cap; ++j) {
                const int n = s_n[j];
                if (n < 1) continue;
                if (n <= left) { s_first[j] = used; used += n; left -= n; }
                else ++skipped;
            }
            s_used = used; s_skipped = skipped;
        }
        __syncthreads();
        // the evasions of the children with rows: lane l owns mask words [6 l, 6 l + 6), so lane order is action order
        for (int j = wave; j < cap; j += kM3Waves) {
            const int first = s_first[j];
            if (first < 0) continue;
            const int n = s_n[j];
            const uint32_t* row = a.c_bits + ((size_t)e * cap + j) * kPlyWords;
            uint32_t m[kM3LaneWords];
            int cnt = 0;
#pragma unroll
            for (int x = 0; x < kM3LaneWords; ++x) {
                const int w = lane * kM3LaneWords + x;
                m[x] = w < kPlyWords ? mask_word(row, w) : 0u;
                cnt += __popc(m[x]);
            }
            int pos = ka_wave_scan(cnt) - cnt;
#pragma unroll
            for (int x = 0; x < kM3LaneWords; ++x) {
                uint32_t b = m[x];
                while (b && pos < n) {                         // (pos < n <= G - first: inside s_act whatever the row holds)
                    s_act[first + pos] = ((lane * kM3LaneWords + x) << 5) + __builtin_ctz(b);
                    s_src[first + pos] = j;
                    ++pos;
                    b &= b - 1u;
                }
            }
        }
        __syncthreads();
    }
    const int used = s_used;
    const long long incoming = a.actions[e];

    if (tid < W) {
        uint32_t word = 0u;
        if (tid == kM3Flags) word = (active ? kM3Active : 0u) | (s_skipped > 0 ? kM3Skipped : 0u);
        else if (tid == kM3Rows) word = (uint32_t)used;
        else if (tid == kM3Slot) word = (uint32_t)-1;
        else if (tid == kM3Action) word = (uint32_t)(int)(incoming < -1 ? -1 : incoming > kPlyA ? kPlyA : incoming);
        else if (tid >= kM3N + cap) word = (uint32_t)s_first[tid - kM3N - cap];
        else if (tid >= kM3N) word = (uint32_t)s_n[tid - kM3N];
        a.rec[(size_t)e * W + tid] = word;
    }

    // ---- the grandchild rows e * G + r: the child's state and new mask for the rows in use, the root's for the others
    // and entries [0, ply + 1) of the child's history rows: an open child is one ply behind its root
    const uint32_t ply = *reinterpret_cast<const uint32_t*>(st + kPlyByte);
    const int hist = a.hist;
    const size_t g0 = (size_t)e * G;
    ply_fork_rows<kM3Threads>(PlyRows{a.g_state + g0 * kStateBytes, a.g_bits + g0 * kPlyWords, a.g_keys + g0 * hist,
                                      a.g_checks + g0 * hist},
                              G, used, hist, (int)min(ply, (uint32_t)hist - 1u) + 1, [&](int r) {
        if (r >= used) return PlyRow{st, lw, nullptr, nullptr};
        const size_t c = (size_t)e * cap + s_src[r];
        return PlyRow{a.c_state + c * kStateBytes, a.c_bits + c * kPlyWords, a.c_keys + c * hist, a.c_checks + c * hist};
    });
    if (tid < G) a.g_actions[g0 + tid] = tid < used ? (long long)s_act[tid] : incoming;
}

// one wave per grandchild row: the first set bit of its new mask, and whether the third ply looks at it
__global__ __launch_bounds__(kM3Threads) void mate3_gate_kernel(Mate3GateArgs a) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * kM3Waves + (threadIdx.x >> 6);
    if (r >= a.rows) return;                                   // (a whole wave: no barrier follows)
    const int e = (int)(r / a.G), i = (int)(r % a.G);
    const uint32_t* rec = a.rec + (size_t)e * m3_words(a.cap);
    const bool on = (rec[kM3Flags] & kM3Active) && i < (int)rec[kM3Rows] && !(a.g_term[r] | a.g_trunc[r]);
    const uint32_t* row = a.g_bits + (size_t)r * kPlyWords;
    int filler = 0;
    for (int w0 = 0; w0 < kPlyWords; w0 += 64) {
        const int w = w0 + lane;
        const uint32_t m = w < kPlyWords ? mask_word(row, w) : 0u;
        const unsigned long long b = __ballot(m != 0u);
        if (b) {
            const int src = __builtin_ctzll(b);
            filler = ((w0 + src) << 5) + __builtin_ctz(__shfl(m, src));
            break;
        }
    }
    if (lane == 0) {
        a.g_model[r] = on ? a.model_of[e] : -1;
        a.g_filler[r] = filler;
    }
}

// one thread per env: at most 64 slots and G grandchild rows each
__global__ __launch_bounds__(kM3Threads) void mate3_choose_kernel(Mate3ChooseArgs a) {
    const int e = blockIdx.x * kM3Threads + threadIdx.x, lane = threadIdx.x & 63;
    const int cap = a.cap, G = a.G, W = m3_words(cap), W1 = mt_words(cap), W3 = mt_words(a.cap3);
    // a refused step moved no row of its launch: its outputs are the unchanged positions, so nothing is chosen from them
    const int held = ((a.err1[0] | a.err1[1]) != 0ull ? 2 : 0) | ((a.err2[0] | a.err2[1]) != 0ull ? 4 : 0) |
                     ((a.err3[0] | a.err3[1]) != 0ull ? 8 : 0);
    bool active = false, mate = false, changed = false;
    int rows = 0, rows3 = 0, skipped = 0;
    if (e < a.n && !held) {
        uint32_t* rec = a.rec + (size_t)e * W;
        const uint32_t* rec1 = a.rec1 + (size_t)e * W1;
        uint32_t flags = rec[kM3Flags];
        if (flags & kM3Active) {
            active = true;
            rows = (int)rec[kM3Rows];
            const int m = a.model_of[e];
            int want3 = 0;
            if (m >= 0 && m < a.K) {
                const int rc = (int)a.table3[(size_t)m * kM3TableWords];
                want3 = rc >= 0 && rc <= kM3MaxCap ? min(rc, a.cap3) : 0;
            }
            const long long incoming = a.actions[e];
            unsigned long long proving = 0ull;
            int first = -1, keep = -1;
            for (int j = 0; j < cap; ++j) {
                const int n = (int)rec[kM3N + j], r0 = (int)rec[kM3N + cap + j];
                if (r0 < 0) {
                    if (n > 0) ++skipped;                      // open, with evasions, without rows
                    continue;
                }
                bool proves = true;
                for (int r = r0; r < r0 + n && r < G; ++r) {
                    const size_t g = (size_t)e * G + r;
                    if (a.g_term[g] | a.g_trunc[g]) { proves = false; continue; }       // refutes, whatever the row now shows
                    const uint32_t* r3 = a.rec3 + g * W3;
                    const uint32_t f3 = r3[kMtFlags];
                    if (f3 & kMtActive) rows3 += (f3 & kMtTruncated) ? want3 : (int)r3[kMtNChecks];
                    if (!(f3 & kMtMate)) {
                        proves = false;
                        if (f3 & kMtTruncated) flags |= kM3Cut3;
                    }
                }
                if (proves) {
                    proving |= 1ull << j;
                    if (first < 0) first = j;                  // (ascending actions: the lowest)
                    if ((long long)(int)rec1[kMtList + j] == incoming) keep = j;
                }
            }
            rec[kM3Proving] = (uint32_t)proving;
            rec[kM3Proving + 1] = (uint32_t)(proving >> 32);
            if (first >= 0) {
                const int slot = keep >= 0 ? keep : first, act = (int)rec1[kMtList + slot];
                mate = true;
                changed = keep < 0;
                rec[kM3Slot] = (uint32_t)slot;
                rec[kM3Action] = (uint32_t)act;
                flags |= kM3Mate | (changed ? kM3Changed : 0u);
                if (changed) a.actions[e] = act;
            }
            rec[kM3Flags] = flags;
        }
    }
    const int na = __popcll(__ballot(active)), nm = __popcll(__ballot(mate)), nc = __popcll(__ballot(changed));
    int nr = rows, n3 = rows3, ns = skipped;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nr += __shfl_xor(nr, o);
        n3 += __shfl_xor(n3, o);
        ns += __shfl_xor(ns, o);
    }
    if (lane == 0) {
        if (na) atomicAdd(&a.stats[0], na);
        if (nr) atomicAdd(&a.stats[1], nr);
        if (n3) atomicAdd(&a.stats[2], n3);
        if (nm) atomicAdd(&a.stats[3], nm);
        if (nc) atomicAdd(&a.stats[4], nc);
        if (ns) atomicAdd(&a.stats[5], ns);
        if (held && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.err[0], held);
    }
}

bool m3_sizes_ok(int cap, int G) { return cap >= 1 && cap <= kM3MaxCap && G >= 1 && G <= kM3MaxRows; }

}  // namespace

extern "C" int ka_mate3_words(int which, int cap) {
    if (cap < 0 || cap > kM3MaxCap) return -1;
    return which == 0 ? m3_words(cap) : which == 1 ? kM3TableWords : which == 2 ? kM3StatsWords + 1 : which == 3 ? kM3MaxRows :
           which == 4 ? kM3MaxCap : -1;
}

extern "C" int ka_mate3_fork(const void* legal, int legal_words, const long long* actions, const int* model_of, int K,
                             const void* table, const void* state, const void* root_records, int cap, const void* child_state,
                             const void* child_keys, const void* child_checks, const void* child_mask_bits,
                             const void* child_terminated, const void* child_truncated, int max_ply, int G, void* records,
                             void* grand_state, void* grand_keys, void* grand_checks, void* grand_mask_bits,
                             long long* grand_actions, int N, int A, void* stream) {
    KA_REQUIRE(legal && actions && model_of && table && state && root_records && child_state && child_keys && child_checks &&
               child_mask_bits && child_terminated && child_truncated && records && grand_state && grand_keys &&
               grand_checks && grand_mask_bits && grand_actions && N > 0, "mate3_fork: null tensor");
    KA_REQUIRE_PLY_SPACE("mate3_fork", A, legal_words);
    KA_REQUIRE(m3_sizes_ok(cap, G), "mate3_fork: cap must lie in [1, %d] and G in [1, %d], got %d and %d", kM3MaxCap,
               kM3MaxRows, cap, G);
    KA_REQUIRE(K >= 1, "mate3_fork: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE_MAX_PLY("mate3_fork", max_ply);
    KA_REQUIRE((long long)N * cap <= INT_MAX && (long long)N * G <= INT_MAX, "mate3_fork: %d envs of %d child and %d "
               "grandchild rows are too many rows", N, cap, G);
    KA_REQUIRE(ka_aligned(16, {legal, state, child_state, child_keys, child_checks, child_mask_bits, grand_state, grand_keys,
                               grand_checks, grand_mask_bits}) &&
               ka_aligned(8, {actions, grand_actions}) && ka_aligned(4, {model_of, table, root_records, records}),
               "mate3_fork: state, history and mask rows are 16-byte aligned, every other tensor to its element size");
    Mate3ForkArgs a{static_cast<const uint32_t*>(legal), actions, model_of, K, static_cast<const uint32_t*>(table),
                    static_cast<const uint8_t*>(state), static_cast<const uint32_t*>(root_records), cap,
                    static_cast<const uint8_t*>(child_state), static_cast<const unsigned long long*>(child_keys),
                    static_cast<const uint8_t*>(child_checks), static_cast<const uint32_t*>(child_mask_bits),
                    static_cast<const uint8_t*>(child_terminated), static_cast<const uint8_t*>(child_truncated),
                    max_ply > 0 ? max_ply : 1, G, static_cast<uint32_t*>(records), static_cast<uint8_t*>(grand_state),
                    static_cast<unsigned long long*>(grand_keys), static_cast<uint8_t*>(grand_checks),
                    static_cast<uint32_t*>(grand_mask_bits), grand_actions};
    hipLaunchKernelGGL(mate3_fork_kernel, dim3(N), dim3(kM3Threads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mate3_fork");
}

extern "C" int ka_mate3_gate(const void* records, int cap, int G, const int* model_of, const void* grand_mask_bits,
                             int legal_words, const void* grand_terminated, const void* grand_truncated, int* grand_model_of,
                             long long* grand_filler, int N, void* stream) {
    KA_REQUIRE(records && model_of && grand_mask_bits && grand_terminated && grand_truncated && grand_model_of &&
               grand_filler && N > 0, "mate3_gate: null tensor");
    KA_REQUIRE(legal_words == kPlyWords, "mate3_gate: packed mask rows of %d words", kPlyWords);
    KA_REQUIRE(m3_sizes_ok(cap, G), "mate3_gate: cap must lie in [1, %d] and G in [1, %d], got %d and %d", kM3MaxCap,
               kM3MaxRows, cap, G);
    KA_REQUIRE((long long)N * G <= INT_MAX, "mate3_gate: %d envs of %d grandchild rows are too many rows", N, G);
    KA_REQUIRE(ka_aligned(4, {records, model_of, grand_mask_bits, grand_model_of}) && ka_aligned(8, {grand_filler}),
               "mate3_gate: every tensor is aligned to its element size");
    const int rows = N * G;
    Mate3GateArgs a{static_cast<const uint32_t*>(records), cap, G, model_of, static_cast<const uint32_t*>(grand_mask_bits),
                    static_cast<const uint8_t*>(grand_terminated), static_cast<const uint8_t*>(grand_truncated),
                    grand_model_of, grand_filler, rows};
    hipLaunchKernelGGL(mate3_gate_kernel, dim3((rows + kM3Waves - 1) / kM3Waves), dim3(kM3Threads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mate3_gate");
}

extern "C" int ka_mate3_choose(void* records, const void* root_records, int cap, int G, const void* third_records, int cap3,
                               const void* grand_terminated, const void* grand_truncated, const int* model_of, int K,
                               const void* third_table, const void* child_err, const void* grand_err, const void* third_err,
                               long long* actions, int* stats, int* err, int N, void* stream) {
    KA_REQUIRE(records && root_records && third_records && grand_terminated && grand_truncated && model_of && third_table &&
               child_err && grand_err && third_err && actions && stats && err && N > 0, "mate3_choose: null tensor");
    KA_REQUIRE(m3_sizes_ok(cap, G), "mate3_choose: cap must lie in [1, %d] and G in [1, %d], got %d and %d", kM3MaxCap,
               kM3MaxRows, cap, G);
    KA_REQUIRE(cap3 >= 1 && cap3 <= kM3MaxCap, "mate3_choose: cap3 must lie in [1, %d], got %d", kM3MaxCap, cap3);
    KA_REQUIRE(K >= 1, "mate3_choose: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE((long long)N * G <= INT_MAX, "mate3_choose: %d envs of %d grandchild rows are too many rows", N, G);
    KA_REQUIRE(ka_aligned(8, {child_err, grand_err, third_err, actions}) &&
               ka_aligned(4, {records, root_records, third_records, model_of, third_table, stats, err}),
               "mate3_choose: actions and the error words are 8-byte aligned, every other tensor to its element size");
    Mate3ChooseArgs a{static_cast<uint32_t*>(records), static_cast<const uint32_t*>(root_records), cap, G,
                      static_cast<const uint32_t*>(third_records), cap3, static_cast<const uint8_t*>(grand_terminated),
                      static_cast<const uint8_t*>(grand_truncated), model_of, K, static_cast<const uint32_t*>(third_table),
                      static_cast<const unsigned long long*>(child_err), static_cast<const unsigned long long*>(grand_err),
                      static_cast<const unsigned long long*>(third_err), actions, stats, err, N};
    hipLaunchKernelGGL(mate3_choose_kernel, dim3((N + kM3Threads - 1) / kM3Threads), dim3(kM3Threads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mate3_choose");
}
