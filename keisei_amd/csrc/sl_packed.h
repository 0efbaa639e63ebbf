// The packed SL record's geometry and the channel pass that packs an observation, shared by sl_pack_kernel (sl_data.hip) and
// the search-sample kernel (search_samples.hip).  The layout itself is stated in sl_data.hip and include/keisei_amd.h.
#pragma once
#include "common.h"

constexpr int kPkThreads = 256;
constexpr int kPkWaves = kPkThreads / 64;
constexpr int kPkChannels = 50;
constexpr int kPkSquares = 81;
constexpr int kPkObsWords = kPkChannels * kPkSquares;         // 4050
constexpr int kPkRowWords = kPkObsWords + 5;                   // 16 220 B: obs, i64 policy, i64 value, f32 score
constexpr int kPkValueAt = 3 * kPkChannels;                    // 150
constexpr int kPkPolicyAt = kPkValueAt + kPkChannels;          // 200
constexpr int kPkWords = kPkPolicyAt + 4;                      // 204
constexpr uint32_t kPkActions = 81 * 139;
static_assert(kPkWords * 4 % 16 == 0, "packed rows are 16-byte aligned");
static_assert(kPkObsWords % 2 == 0, "the gather stores pairs");

// The channel pass of a workgroup of kPkThreads: wave w takes channels w, w + 4, ... of the 4050 observation words at src
// and writes their three mask words and their value word into the row staged in LDS.  Returns whether a channel of this
// wave held two different non-zero patterns (the observation cannot be held packed).  Every lane of every wave must call
// it: the bounds are wave-uniform and all 64 lanes reach every ballot.
__device__ __forceinline__ bool sl_pack_channels(const uint32_t* __restrict__ src, uint32_t* s_row, int lane, int wave) {
    bool bad = false;
    for (int c = wave; c < kPkChannels; c += kPkWaves) {
        const uint32_t* plane = src + c * kPkSquares;
        const uint32_t x0 = plane[lane];
        const uint32_t x1 = lane < kPkSquares - 64 ? plane[64 + lane] : 0u;
        const unsigned long long m0 = __ballot(x0 != 0u), m1 = __ballot(x1 != 0u);
        const uint32_t v0 = __shfl(x0, m0 ? __ffsll(m0) - 1 : 0);
        const uint32_t v1 = __shfl(x1, m1 ? __ffsll(m1) - 1 : 0);
        const uint32_t value = m0 ? v0 : v1;                      // (no set lane at all: x1 of lane 0, which is 0)
        bad |= __ballot((x0 != 0u && x0 != value) || (x1 != 0u && x1 != value)) != 0ull;
        if (lane == 0) {
            s_row[3 * c + 0] = (uint32_t)m0;
            s_row[3 * c + 1] = (uint32_t)(m0 >> 32);
            s_row[3 * c + 2] = (uint32_t)m1;
            s_row[kPkValueAt + c] = value;
        }
    }
    return bad;
}
