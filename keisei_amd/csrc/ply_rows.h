// The rows the searches of the device ply read and fork: the spatial action space, the packed mask row over it, and the
// one copy that makes child rows out of env rows.  The lookahead, its reply search and the tree search (csrc/lookahead.hip),
// the mate in one (csrc/mate.hip) and the mate in three (csrc/mate3.hip) fork through ply_fork_rows; the policy insight
// (csrc/insight.hip) takes the action space and the mask row from here.  The state row is csrc/shogi_rules.h's.
#pragma once
#include "shogi_rules.h"

constexpr int kPlySlots = 139, kPlyA = 81 * kPlySlots;                            // the spatial action space, 81 * 139 = 11 259
constexpr int kPlyWords = (kPlyA + 31) / 32;                                      // 32-bit words of a packed mask row
constexpr uint32_t kPlyTailBits = (1u << (kPlyA - 32 * (kPlyWords - 1))) - 1u;    // the bits of the last word that are actions
constexpr int kPlyStateUnits = kStateBytes / 16, kPlyMaskUnits = kPlyWords * 4 / 16;    // 16-byte pieces of a state / mask row
static_assert(kPlyWords * 4 % 16 == 0 && kStateBytes % 16 == 0, "state and mask rows are copied in 16-byte pieces");

// word w of a mask row; bits past the action space are dropped, so no index taken from it reaches A
__device__ __forceinline__ uint32_t mask_word(const uint32_t* row, int w) {
    return w == kPlyWords - 1 ? row[w] & kPlyTailBits : row[w];
}

// the launchers' checks of the action space, the mask rows and max_ply, under the entry point's own name (host side; they
// stand here because they need kPlyA and kPlyWords)
#define KA_REQUIRE_PLY_SPACE(who, A, legal_words)                                                                  \
    do {                                                                                                           \
        KA_REQUIRE((A) == kPlyA, who ": the spatial action space only (A = %d), got %d", kPlyA, (A));              \
        KA_REQUIRE((legal_words) == kPlyWords, who ": packed mask rows of %d words", kPlyWords);                   \
    } while (0)
#define KA_REQUIRE_MAX_PLY(who, max_ply)                                                                       \
    KA_REQUIRE((max_ply) >= 0 && (max_ply) <= 65535, who ": max_ply must lie in [0, 65535], got %d", (max_ply))

struct PlyRow { const uint8_t* state; const uint32_t* bits; const unsigned long long* keys; const uint8_t* checks; };     // one row read
struct PlyRows { uint8_t* state; uint32_t* bits; unsigned long long* keys; uint8_t* checks; };     // a workgroup's rows written, row 0 first

// `units` pieces of type T from the history row src(r) to row r of dst, for the rows [0, used)
template <int THREADS, class T, class E, class Src>
__device__ __forceinline__ void ply_copy_history(E* dst, int hist, int units, int used, Src src) {
    for (int u = threadIdx.x; u < units * used; u += THREADS) {
        const int r = u / units, p = u % units;
        reinterpret_cast<T*>(dst + (size_t)r * hist)[p] = reinterpret_cast<const T*>(src(r))[p];
    }
}

// The fork copy of a workgroup of THREADS threads: row r of dst gets the state and the mask of src_of(r) for every r in
// [0, rows), and entries [0, n) of its key and check history for the rows in use, r in [0, used) -- the env kernel only
// counts repetitions in the history, and nothing reads the outcome of an unused row.  Every thread takes part, 16 bytes per
// lane where the rows allow it: rows of an even number of keys start at 16-byte boundaries (an odd count takes one stale key
// along: it stays inside the row), check rows go in 16-, 4- or 1-byte pieces by the same rule.  src_of(r) is a PlyRow; its
// history pointers are read for r < used only.
template <int THREADS, class SrcOf>
__device__ __forceinline__ void ply_fork_rows(const PlyRows& dst, int rows, int used, int hist, int n, SrcOf src_of) {
    constexpr int kUnits = kPlyStateUnits + kPlyMaskUnits;
    for (int u = threadIdx.x; u < kUnits * rows; u += THREADS) {
        const int r = u / kUnits, p = u % kUnits;
        const PlyRow s = src_of(r);
        if (p < kPlyStateUnits) reinterpret_cast<uint4*>(dst.state + (size_t)r * kStateBytes)[p] = reinterpret_cast<const uint4*>(s.state)[p];
        else reinterpret_cast<uint4*>(dst.bits + (size_t)r * kPlyWords)[p - kPlyStateUnits] = reinterpret_cast<const uint4*>(s.bits)[p - kPlyStateUnits];
    }
    if (used <= 0 || n <= 0) return;
    const auto keys = [&](int r) { return src_of(r).keys; };
    const auto checks = [&](int r) { return src_of(r).checks; };
    if ((hist & 1) == 0) ply_copy_history<THREADS, uint4>(dst.keys, hist, (n + 1) >> 1, used, keys);
    else ply_copy_history<THREADS, unsigned long long>(dst.keys, hist, n, used, keys);
    if ((hist & 15) == 0) ply_copy_history<THREADS, uint4>(dst.checks, hist, (n + 15) >> 4, used, checks);
    else if ((hist & 3) == 0) ply_copy_history<THREADS, uint32_t>(dst.checks, hist, (n + 3) >> 2, used, checks);
    else ply_copy_history<THREADS, uint8_t>(dst.checks, hist, n, used, checks);
}
