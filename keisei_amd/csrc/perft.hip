// Perft on the device: fork every legal move of a frontier of positions, step the children with the env kernel as it is,
// count.  The mate searches fork a capped few moves of one env; this is the full-width fork -- all set bits of a mask row,
// for a whole frontier of parents, the children placed by a scan over the parents -- and perft is its first user, the one
// with an exact integer oracle.  A level of the walk is a set of complete env rows (state, history, mask), so the stages are
//
//   ka_perft_tally          over the rows just stepped (or the env's own): moves[row] = the set bits of the row's new mask,
//                           0 where the game ended; nodes / mates / other endings / checks into tally[tag[row]][level];
//                           with `leaf` the moves into leaves[tag[row]] (bulk counting: the last level is never forked)
//   ka_perft_plan           one workgroup over moves[cursor .. n): the longest prefix of whole parents whose children fit
//                           `cap` rows, offset[p] for each, and a header {taken, children, blocking row or -1} for the host
//   ka_perft_fork           one workgroup per taken parent: child row offset[p] + rank for the rank-th set bit of the
//                           parent's mask, ascending: state, history, the parent's mask, action, tag
//   ka_shogi_env_step       (csrc/shogi_env.hip, unchanged) over exactly `children` rows
//
// and the host walks the tree depth-first over chunks (keisei_amd/perft.py).  This is perft under the env's game rules: a
// row whose game ended has no successors (the step has restarted it: its state and mask are a fresh game's, which is why
// `moves` and not the mask decides who is forked).  The parents are only read and may not alias the children.  Kernel nodes
// only, caller-owned buffers, no workgroup waits for another.  Counters are 64-bit and added to with plain atomicAdd, once
// per run of equal tags in a wave: the rows of one tag are mostly contiguous.
#include "ply_rows.h"

#include <climits>

namespace {

constexpr int kPfThreads = 256, kPfWaves = kPfThreads / 64;
constexpr int kPfPlanThreads = 1024, kPfPlanWaves = kPfPlanThreads / 64;
constexpr int kPfTallyRows = 64;                                // rows of a tally workgroup: one lane of wave 0 each
constexpr int kPfCols = 4, kPfHeader = 3;                       // nodes, mates, other endings, checks; taken, children, blocking row
constexpr int kPfMaxMoves = 593, kPfMaxCap = 1 << 20, kPfMaxDepth = 8;      // (1024 clamped counts of a plan tile sum within an int)

struct PerftTallyArgs {
    const uint8_t* state; const uint32_t* bits; const uint8_t* term; const uint8_t* trunc; const uint8_t* reason; const int* tag;
    int n, level, depth, leaf, tags;
    int* moves; unsigned long long* tally; unsigned long long* leaves;
};

struct PerftForkArgs {
    const uint8_t* state; const uint32_t* bits; const unsigned long long* keys; const uint8_t* checks;
    const int* moves; const int* offset; const int* tag;
    int cursor, hist, cap, divide_base;
    uint8_t* c_state; unsigned long long* c_keys; uint8_t* c_checks; uint32_t* c_bits; long long* c_actions; int* c_tag; int* err;
};

// 64 rows per workgroup.  Every wave counts the mask rows of 16 of them, 16 bytes per lane; wave 0 then holds one row per
// lane and adds the counts of each run of equal tags with one atomic per column.
__global__ __launch_bounds__(kPfThreads) void perft_tally_kernel(PerftTallyArgs a) {
    __shared__ int s_moves[kPfTallyRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * kPfTallyRows;
    for (int j = wave; j < kPfTallyRows; j += kPfWaves) {
        const int r = row0 + j;
        if (r >= a.n) break;                                   // (uniform over the wave)
        int cnt = 0;
        if (!(a.term && (a.term[r] | a.trunc[r]))) {
            const uint32_t* lw = a.bits + (size_t)r * kPlyWords;
            for (int u = lane; u < kPlyMaskUnits; u += 64) {
                const uint4 v = reinterpret_cast<const uint4*>(lw)[u];
                cnt += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(u == kPlyMaskUnits - 1 ? v.w & kPlyTailBits : v.w);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        }
        if (lane == 0) s_moves[j] = cnt;
    }
    __syncthreads();
    if (wave != 0) return;
    const int r = row0 + lane;
    const bool valid = r < a.n;
    int mv = 0, t = -1;
    bool mate = false, other = false, check = false;
    if (valid) {
        const bool ended = a.term && (a.term[r] | a.trunc[r]);
        mate = ended && a.reason[r] == R_CHECKMATE;
        other = ended && !mate;
        check = a.state[(size_t)r * kStateBytes + kCheckByte] != 0;
        mv = s_moves[lane];
        a.moves[r] = mv;
        t = a.tag[r];
    }
    unsigned long long todo = __ballot(valid && t >= 0 && t < a.tags);       // (a tag outside the table counts nowhere)
    while (todo) {                                             // (uniform over the wave)
        const int leader = __ffsll((long long)todo) - 1;
        const int lt = __shfl(t, leader);
        const bool mine = ((todo >> lane) & 1ull) && t == lt;
        const unsigned long long grp = __ballot(mine);
        const int nm = __popcll(__ballot(mine && mate)), no = __popcll(__ballot(mine && other));
        const int nc = __popcll(__ballot(mine && check));
        int sum = mine ? mv : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == leader) {
            if (a.level >= 0) {
                unsigned long long* row = a.tally + ((size_t)lt * a.depth + a.level) * kPfCols;
                atomicAdd(&row[0], (unsigned long long)__popcll(grp));
                if (nm) atomicAdd(&row[1], (unsigned long long)nm);
                if (no) atomicAdd(&row[2], (unsigned long long)no);
                if (nc) atomicAdd(&row[3], (unsigned long long)nc);
            }
            if (a.leaf && sum) atomicAdd(&a.leaves[lt], (unsigned long long)sum);
        }
        todo &= ~grp;
    }
}

// One workgroup.  Tiles of 1024 parents from `cursor`; a parent fits when the children before it plus its own are at most
// `cap`.  Counts are not negative, so the parents that fit are a prefix, and the walk stops at the first tile that holds
// one that does not.  Counts are clamped to cap + 1 (and cap to 2^20), which changes no decision and keeps a tile's sum
// inside an int.
__global__ __launch_bounds__(kPfPlanThreads) void perft_plan_kernel(const int* moves, int cursor, int n, int cap, int* offset,
                                                                    int* header) {
    __shared__ int s_wave[kPfPlanWaves];
    __shared__ int s_red[kPfPlanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int running = 0, taken = 0;                                // children and parents so far (running <= cap)
    for (int base = cursor; base < n; base += kPfPlanThreads) {
        const int i = base + tid;
        const int v = i < n ? min(max(moves[i], 0), cap + 1) : 0;
        const int inc = ka_wave_scan(v);
        __syncthreads();                                       // (the tile before has read s_wave)
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int pre = inc - v;
        for (int x = 0; x < wave; ++x) pre += s_wave[x];
        const bool fits = i < n && (long long)running + pre + v <= (long long)cap;
        if (fits) offset[i] = running + pre;
        const int c = ka_block_sum<kPfPlanThreads>(fits ? 1 : 0, s_red);
        const int kids = ka_block_sum<kPfPlanThreads>(fits ? v : 0, s_red);
        taken += c;
        running += kids;
        if (c < min(kPfPlanThreads, n - base)) break;          // (uniform: every thread has the same c)
    }
    if (tid == 0) {
        const int stop = cursor + taken;
        header[0] = taken;
        header[1] = running;
        header[2] = cursor >= 0 && stop < n && moves[stop] > cap ? stop : -1;
    }
}

// One workgroup per taken parent.  A pass is 256 consecutive mask words, one per thread: thread order is action order, so
// an exclusive block scan of the popcounts ranks every set bit.  moves[p] is the authority on how many children the parent
// has (0: its game ended, whatever its mask shows); a mask that disagrees, or children that would leave the `cap` rows,
// set err and write nothing outside their rows.
__global__ __launch_bounds__(kPfThreads) void perft_fork_kernel(PerftForkArgs a) {
    __shared__ int s_wave[kPfWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = a.cursor + blockIdx.x;
    const int mv = a.moves[p];
    if (mv <= 0) return;                                       // (uniform over the workgroup, as every branch below)
    const int off = a.offset[p];
    if (off < 0 || off > a.cap - mv) {
        if (tid == 0) atomicOr(a.err, 1);
        return;
    }
    const uint32_t* lw = a.bits + (size_t)p * kPlyWords;
    const uint8_t* st = a.state + (size_t)p * kStateBytes;
    const int tag = a.tag[p];
    int found = 0;
    for (int w0 = 0; w0 < kPlyWords; w0 += kPfThreads) {
        const int w = w0 + tid;
        uint32_t m = w < kPlyWords ? mask_word(lw, w) : 0u;
        const int cnt = __popc(m), inc = ka_wave_scan(cnt);
        __syncthreads();                                       // (the pass before has read s_wave)
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int pos = found + inc - cnt, total = 0;
        for (int x = 0; x < kPfWaves; ++x) {
            if (x < wave) pos += s_wave[x];
            total += s_wave[x];
        }
        while (m && pos < mv) {
            const int c = off + pos++;
            a.c_actions[c] = (long long)((w << 5) + __builtin_ctz(m));
            a.c_tag[c] = a.divide_base >= 0 ? a.divide_base + c : tag;
            m &= m - 1u;
        }
        found += total;
    }
    if (found != mv && tid == 0) atomicOr(a.err, 2);
    const int hist = a.hist;
    const uint32_t ply = *reinterpret_cast<const uint32_t*>(st + kPlyByte);
    const PlyRow parent{st, lw, a.keys + (size_t)p * hist, a.checks + (size_t)p * hist};
    ply_fork_rows<kPfThreads>(PlyRows{a.c_state + (size_t)off * kStateBytes, a.c_bits + (size_t)off * kPlyWords,
                                      a.c_keys + (size_t)off * hist, a.c_checks + (size_t)off * hist},
                              mv, mv, hist, (int)min(ply, (uint32_t)hist), [&](int) { return parent; });
}

// do [a, a + na) and [b, b + nb) share no byte?
bool pf_apart(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + na <= y || y + nb <= x;
}

}  // namespace

extern "C" int ka_perft_words(int which) {
    return which == 0 ? kPfCols : which == 1 ? kPfHeader : which == 2 ? kPfMaxMoves : which == 3 ? kPfMaxCap : which == 4 ? kPfMaxDepth : -1;
}

extern "C" int ka_perft_tally(const void* state, const void* mask_bits, int legal_words, const void* terminated,
                              const void* truncated, const void* reason, const int* tag, int n, int level, int depth, int leaf,
                              int tags, int* moves, void* tally, void* leaves, void* stream) {
    KA_REQUIRE(state && mask_bits && tag && moves && n > 0, "perft_tally: null tensor");
    KA_REQUIRE(legal_words == kPlyWords, "perft_tally: packed mask rows of %d words", kPlyWords);
    KA_REQUIRE((terminated != nullptr) == (truncated != nullptr) && (terminated != nullptr) == (reason != nullptr),
               "perft_tally: terminated, truncated and reason are all given (rows just stepped) or all NULL (the env's own)");
    KA_REQUIRE(depth >= 1 && depth <= kPfMaxDepth && level >= -1 && level < depth && tags >= 1,
               "perft_tally: depth in [1, %d], level in [-1, depth), tags >= 1; got %d, %d, %d", kPfMaxDepth, depth, level, tags);
    KA_REQUIRE((level < 0 || tally) && (!leaf || leaves), "perft_tally: a level needs the tally table, a leaf level the leaves");
    KA_REQUIRE(ka_aligned(16, {state, mask_bits}) && ka_aligned(8, {tally, leaves}) && ka_aligned(4, {tag, moves}),
               "perft_tally: state and mask rows are 16-byte aligned, every other tensor to its element size");
    PerftTallyArgs a{static_cast<const uint8_t*>(state), static_cast<const uint32_t*>(mask_bits),
                     static_cast<const uint8_t*>(terminated), static_cast<const uint8_t*>(truncated),
                     static_cast<const uint8_t*>(reason), tag, n, level, depth, leaf != 0, tags, moves,
                     static_cast<unsigned long long*>(tally), static_cast<unsigned long long*>(leaves)};
    hipLaunchKernelGGL(perft_tally_kernel, dim3((n + kPfTallyRows - 1) / kPfTallyRows), dim3(kPfThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("perft_tally");
}

extern "C" int ka_perft_plan(const int* moves, int cursor, int n, int cap, int* offset, int* header, void* stream) {
    KA_REQUIRE(moves && offset && header, "perft_plan: null tensor");
    KA_REQUIRE(n >= 0 && cursor >= 0 && cursor <= n, "perft_plan: cursor must lie in [0, n], got %d of %d", cursor, n);
    KA_REQUIRE(cap >= 1 && cap <= kPfMaxCap, "perft_plan: cap must lie in [1, %d], got %d", kPfMaxCap, cap);
    KA_REQUIRE(ka_aligned(4, {moves, offset, header}), "perft_plan: tensors are aligned to their 32-bit words");
    hipLaunchKernelGGL(perft_plan_kernel, dim3(1), dim3(kPfPlanThreads), 0, static_cast<hipStream_t>(stream), moves, cursor, n,
                       cap, offset, header);
    return ka_check_launch("perft_plan");
}

extern "C" int ka_perft_fork(const void* state, const void* mask_bits, int legal_words, const void* keys, const void* checks,
                             const int* moves, const int* offset, const int* tag, int cursor, int taken, int n, int max_ply,
                             int cap, int divide_base, void* child_state, void* child_keys, void* child_checks,
                             void* child_mask_bits, long long* child_actions, int* child_tag, int* err, int A, void* stream) {
    KA_REQUIRE(state && mask_bits && keys && checks && moves && offset && tag && child_state && child_keys && child_checks &&
               child_mask_bits && child_actions && child_tag && err, "perft_fork: null tensor");
    KA_REQUIRE_PLY_SPACE("perft_fork", A, legal_words);
    KA_REQUIRE_MAX_PLY("perft_fork", max_ply);
    KA_REQUIRE(cap >= 1 && cap <= kPfMaxCap, "perft_fork: cap must lie in [1, %d], got %d", kPfMaxCap, cap);
    KA_REQUIRE(n >= 1 && cursor >= 0 && taken >= 1 && taken <= n - cursor,
               "perft_fork: the parents [cursor, cursor + taken) lie in [0, n); got cursor %d, taken %d, n %d", cursor, taken, n);
    KA_REQUIRE(divide_base >= -1 && (long long)divide_base + cap <= INT_MAX, "perft_fork: divide_base is -1 or a first ordinal");
    KA_REQUIRE(ka_aligned(16, {state, mask_bits, keys, checks, child_state, child_keys, child_checks, child_mask_bits}) &&
               ka_aligned(8, {child_actions}) && ka_aligned(4, {moves, offset, tag, child_tag, err}),
               "perft_fork: state, history and mask rows are 16-byte aligned, every other tensor to its element size");
    const size_t hist = max_ply > 0 ? max_ply : 1, np = (size_t)n, nc = (size_t)cap;
    KA_REQUIRE(pf_apart(state, np * kStateBytes, child_state, nc * kStateBytes) &&
               pf_apart(mask_bits, np * kPlyWords * 4, child_mask_bits, nc * kPlyWords * 4) &&
               pf_apart(keys, np * hist * 8, child_keys, nc * hist * 8) && pf_apart(checks, np * hist, child_checks, nc * hist) &&
               pf_apart(tag, np * 4, child_tag, nc * 4),
               "perft_fork: the parents' rows are only read and may not overlap the children's");
    PerftForkArgs a{static_cast<const uint8_t*>(state), static_cast<const uint32_t*>(mask_bits),
                    static_cast<const unsigned long long*>(keys), static_cast<const uint8_t*>(checks), moves, offset, tag,
                    cursor, (int)hist, cap, divide_base, static_cast<uint8_t*>(child_state),
                    static_cast<unsigned long long*>(child_keys), static_cast<uint8_t*>(child_checks),
                    static_cast<uint32_t*>(child_mask_bits), child_actions, child_tag, err};
    hipLaunchKernelGGL(perft_fork_kernel, dim3(taken), dim3(kPfThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("perft_fork");
}
