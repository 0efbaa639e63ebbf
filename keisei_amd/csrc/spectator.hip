// Spectator feed: the per-env move history of the reference's VecEnv (vec_env.rs:259, 618-622, 693-714) with what its
// Hodges notation needs (spectator_data.rs:105-186), computed where the position and the legal moves are: on the device,
// at the moment of the move.  The game log (gamelog.hip) keeps bare action indices; the notation of a move also needs the
// piece that moves, whether it captures, whether it could promote, and which other pieces of its kind could reach the
// same square.  All of that is packed into one uint32 note per move; the host turns notes into text (shogi_gym.py).
//
// Note, from bit 0: action index (14 bits), mover's colour, piece type (4 bits: 1 P .. 8 K; for a drop the dropped type),
// the piece is already promoted, drop, capture, promotion suffix class (2 bits: 0 none, 1 '+', 2 '='), disambiguation class
// (2 bits: 0 none, 1 file, 2 rank, 3 full square), no piece on `from`.  An action outside the action space gives 0; one
// inside it that points off the board gives the bare action index (the env refuses both, the note is never committed).
//
// spectator_note_kernel runs BEFORE the env step: one wave per env reads the state row, the packed mask row the action is
// validated against, and the action.  The "others" of spectator_data.rs:132-145 are found without generating moves: a
// square that holds the mover's piece byte is an other when the action index of its move to the same square (plain or
// promoting) is set in the mask row -- the mask is exact, blockers, pins and checks are resolved in it.
// spectator_commit_kernel runs AFTER the env step: nothing happens when the step was refused (err[0] != 0); otherwise the
// pending note is appended to the env's row and the rows of the envs that finished are emptied (their count becomes 0).
// Kernel nodes only, caller-owned buffers, no atomics, no workgroup waits for another.
#include "shogi_rules.h"

namespace {

constexpr int kSpThreads = 256;
constexpr int kSpTypes = 139, kSpBoardMoves = 81 * 80 * 2;
constexpr int kSpActionBits = 14, kSpColour = 14, kSpType = 15, kSpPromoted = 19, kSpDrop = 20, kSpCapture = 21,
              kSpSuffix = 22, kSpDisamb = 24, kSpNoPiece = 26;
constexpr int kSpKing = 8, kSpGold = 5, kSpWhite = 0x10, kSpProm = 0x20;

__host__ __device__ constexpr int sp_action_space(int amode) { return amode ? 81 * kSpTypes : kSpBoardMoves + 81 * 7; }
// the eight directions of spatial_action_mapper.rs:31-40 (N NE E SE S SW W NW), as shogi_env.hip has them
__device__ __forceinline__ int sp_dr(int d) { return ((0x1A90 >> (2 * d)) & 3) - 1; }
__device__ __forceinline__ int sp_dc(int d) { return ((0x01A9 >> (2 * d)) & 3) - 1; }
// direction index of a unit step (ur, uc), a nibble per (ur + 1) * 3 + uc + 1
__device__ __forceinline__ int sp_dir_of(int ur, int uc) { return (int)((0x345206107ull >> (4 * ((ur + 1) * 3 + uc + 1))) & 15); }

__global__ __launch_bounds__(kSpThreads) void spectator_note_kernel(const uint8_t* state, int state_bytes, int E,
                                                                    const uint32_t* bits, const long long* actions, int amode,
                                                                    uint32_t* pending) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * (kSpThreads / 64) + (threadIdx.x >> 6);
    if (e >= E) return;                                        // (uniform over the wave)
    const int A = sp_action_space(amode), words = (A + 31) >> 5;
    const uint8_t* st = state + (size_t)e * state_bytes;
    const uint32_t* row = bits + (size_t)e * words;
    const long long act64 = actions[e];
    uint32_t note = 0;
    if (act64 >= 0 && act64 < A) {                             // every branch on the action is uniform over the wave
        const int act = (int)act64, side = st[kSideByte] & 1;
        // decode in the mover's perspective (spatial_action_mapper.rs:188-279 / action_mapper.rs:79-110)
        int from_p = 0, to_p = 0, promote = 0, drop = -1;
        bool on_board = true;
        if (amode) {
            const int slot = act % kSpTypes;
            from_p = act / kSpTypes;
            int r, c;
            if (slot < 128) {
                promote = slot >= 64;
                const int b = slot & 63, d = b >> 3, dist = (b & 7) + 1;
                r = from_p / 9 + sp_dr(d) * dist; c = from_p % 9 + sp_dc(d) * dist;
            } else if (slot < 132) {
                const int k = slot - 128;
                promote = k & 1; r = from_p / 9 - 2; c = from_p % 9 + ((k >> 1) ? 1 : -1);
            } else { drop = slot - 132; r = from_p / 9; c = from_p % 9; }
            on_board = (unsigned)r < 9u && (unsigned)c < 9u;
            to_p = r * 9 + c;
        } else if (act < kSpBoardMoves) {
            from_p = act / 160;
            const int rem = act % 160, off = rem >> 1;
            promote = rem & 1; to_p = off >= from_p ? off + 1 : off;
        } else { drop = (act - kSpBoardMoves) % 7; to_p = from_p = (act - kSpBoardMoves) / 7; }
        note = (uint32_t)act;
        if (on_board) {
            const int to = side ? 80 - to_p : to_p;
            note |= (uint32_t)side << kSpColour;
            if (drop >= 0) {
                note |= ((uint32_t)(drop + 1) << kSpType) | (1u << kSpDrop);
            } else {
                const int from = side ? 80 - from_p : from_p;
                const int pc = st[from];
                if (st[to]) note |= 1u << kSpCapture;
                if (!pc) {
                    note |= 1u << kSpNoPiece;                  // the reference's "?5e-5d" (spectator_data.rs:112-115)
                } else {
                    const int t = pc & 15, prom = (pc & kSpProm) ? 1 : 0;
                    const int from_row = from / 9, to_row = to / 9;
                    const bool must = (t == 1 || t == 2) ? (side ? to_row == 8 : to_row == 0)          // movegen.rs:35-47
                                    : t == 3 ? (side ? to_row >= 7 : to_row <= 1) : false;
                    const bool can = !prom && t != kSpGold && t != kSpKing;
                    const bool zone = side ? (from_row >= 6 || to_row >= 6) : (from_row <= 2 || to_row <= 2);
                    const int suffix = (promote || must) ? 1 : (can && zone) ? 2 : 0;
                    bool other = false, same_file = false, same_rank = false;
                    if (t != kSpKing) {
                        for (int sq = lane; sq < 81; sq += 64) {
                            if (sq == from || sq == to || st[sq] != pc) continue;
                            const int f_p = side ? 80 - sq : sq;
                            int a0 = -1, pstep = 1;
                            if (amode) {
                                const int dr = to_p / 9 - f_p / 9, dc = to_p % 9 - f_p % 9;
                                const int adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
                                if (dr == 0 || dc == 0 || adr == adc) {
                                    const int d = sp_dir_of((dr > 0) - (dr < 0), (dc > 0) - (dc < 0));
                                    a0 = f_p * kSpTypes + d * 8 + max(adr, adc) - 1;
                                    pstep = 64;
                                } else if (dr == -2 && adc == 1) {
                                    a0 = f_p * kSpTypes + 128 + (dc > 0 ? 2 : 0);
                                }
                            } else {
                                a0 = f_p * 160 + (to_p > f_p ? to_p - 1 : to_p) * 2;
                            }
                            if (a0 < 0) continue;
                            const int a1 = a0 + pstep;         // (both below A: a slot below 132, an offset below 160)
                            if ((((row[a0 >> 5] >> (a0 & 31)) | (row[a1 >> 5] >> (a1 & 31))) & 1u) == 0) continue;
                            other = true;
                            same_file |= sq % 9 == from % 9;
                            same_rank |= sq / 9 == from_row;
                        }
                    }
                    const bool any = __ballot(other) != 0, sf = __ballot(same_file) != 0, sr = __ballot(same_rank) != 0;
                    const int disamb = !any ? 0 : !sf ? 1 : !sr ? 2 : 3;
                    note |= ((uint32_t)t << kSpType) | ((uint32_t)prom << kSpPromoted) | ((uint32_t)suffix << kSpSuffix) |
                            ((uint32_t)disamb << kSpDisamb);
                }
            }
        }
    }
    if (lane == 0) pending[e] = note;
}

__global__ __launch_bounds__(kSpThreads) void spectator_commit_kernel(const long long* err, const uint8_t* terminated,
                                                                      const uint8_t* truncated, int E, const uint32_t* pending,
                                                                      uint32_t* hist, int row_len, int* count) {
    const int e = blockIdx.x * kSpThreads + threadIdx.x;
    if (e >= E || err[0] != 0) return;                         // a refused step moved no game: no history changes
    const int c = max(count[e], 0);
    if (c < row_len) hist[(size_t)e * row_len + c] = pending[e];
    count[e] = (terminated[e] | truncated[e]) ? 0 : min(c + 1, row_len);
}

__global__ __launch_bounds__(kSpThreads) void spectator_begin_kernel(int E, int* count) {
    const int e = blockIdx.x * kSpThreads + threadIdx.x;
    if (e < E) count[e] = 0;
}

}  // namespace

extern "C" int ka_spectator_words(int which) {
    return which == 0 ? kSpActionBits : which == 1 ? kSpColour : which == 2 ? kSpType : which == 3 ? kSpPromoted
         : which == 4 ? kSpDrop : which == 5 ? kSpCapture : which == 6 ? kSpSuffix : which == 7 ? kSpDisamb
         : which == 8 ? kSpNoPiece : which == 9 ? 1 : -1;
}

extern "C" int ka_spectator_begin(int* count, int envs, void* stream) {
    KA_REQUIRE(count && envs > 0, "spectator_begin: null count or envs %d", envs);
    hipLaunchKernelGGL(spectator_begin_kernel, dim3((envs + kSpThreads - 1) / kSpThreads), dim3(kSpThreads), 0,
                       static_cast<hipStream_t>(stream), envs, count);
    return ka_check_launch("spectator_begin");
}

extern "C" int ka_spectator_note(const void* env_state, int state_bytes, int envs, const void* mask_bits,
                                 const long long* actions, int action_mode, void* pending, void* stream) {
    KA_REQUIRE(env_state && mask_bits && actions && pending, "spectator_note: null tensor");
    KA_REQUIRE(envs > 0 && state_bytes >= 96, "spectator_note: envs %d, state rows of %d bytes (at least 96)", envs, state_bytes);
    KA_REQUIRE(action_mode == 0 || action_mode == 1, "spectator_note: action_mode is 0 (default) or 1 (spatial)");
    KA_REQUIRE((uintptr_t)mask_bits % 4 == 0 && (uintptr_t)pending % 4 == 0, "spectator_note: mask_bits and pending are 4-byte aligned");
    const int per = kSpThreads / 64;
    hipLaunchKernelGGL(spectator_note_kernel, dim3((envs + per - 1) / per), dim3(kSpThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(env_state), state_bytes, envs, static_cast<const uint32_t*>(mask_bits), actions,
                       action_mode, static_cast<uint32_t*>(pending));
    return ka_check_launch("spectator_note");
}

extern "C" int ka_spectator_commit(const void* err, const void* terminated, const void* truncated, int envs,
                                   const void* pending, void* hist, int row_len, int* count, void* stream) {
    KA_REQUIRE(err && terminated && truncated && pending && hist && count, "spectator_commit: null tensor");
    KA_REQUIRE(envs > 0 && row_len > 0, "spectator_commit: envs %d, row_len %d", envs, row_len);
    KA_REQUIRE((uintptr_t)err % 8 == 0 && (uintptr_t)hist % 4 == 0 && (uintptr_t)pending % 4 == 0,
               "spectator_commit: err is 8-byte aligned, hist and pending 4-byte aligned");
    hipLaunchKernelGGL(spectator_commit_kernel, dim3((envs + kSpThreads - 1) / kSpThreads), dim3(kSpThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const long long*>(err),
                       static_cast<const uint8_t*>(terminated), static_cast<const uint8_t*>(truncated), envs,
                       static_cast<const uint32_t*>(pending), static_cast<uint32_t*>(hist), row_len, count);
    return ka_check_launch("spectator_commit");
}
