// The packed, device-resident SL dataset (keisei_amd/sl/device_dataset.py).  A shard record is 4050 floats of observation, but
// each of its 50 channels is a 0/1 piece plane or a spatially constant plane: the non-zero squares of a plane share one
// 32-bit pattern.  Three mask words and one value word per channel reproduce the observation bit for bit -- 816 bytes
// instead of 16 220 -- so a whole corpus stays in HBM and a minibatch is one launch with no host work.
//
// Packed record, KA_SL_PACKED_WORDS = 204 dwords (include/keisei_amd.h is the contract):
//   [3c, 3c+3)  occupancy of channel c: bit p of the 96-bit little-endian field is set iff the PATTERN of obs[c*81 + p] is
//               non-zero (-0.0 is non-zero); bits 81..95 are zero
//   150 + c     the pattern the non-zero squares of channel c share, 0 for an empty mask
//   200, 201    policy, value (int32);  202 the score's bits;  203 zero
//
//   sl_pack_kernel    one workgroup per record, wave w takes channels w, w+4, ...: lanes load squares 0..63 and 64..80, two
//                     ballots are the mask, the value is the pattern of the lowest set lane, a third ballot (non-zero and
//                     not the value) says whether the record can be held packed at all.  The 204 words go through LDS and
//                     out in one coalesced store.  A source row starts at 16 220 * r bytes, 8-byte aligned only for even r:
//                     every load is a 4-byte load, the int64 targets as two dwords each.
//   sl_gather_kernel  one workgroup per batch row: the 816 bytes of row idx[b] into LDS, then the 16 200-byte NCHW fp32
//                     observation as coalesced 8-byte stores (a row of obs_out starts at 16 200 * b bytes: 8-byte aligned
//                     only) and the three targets.  An index outside [0, n) counts in the flag word and gives a zero row:
//                     nothing outside the dataset is read.
//   sl_gather_kernel<true> (ka_sl_gather_aug) is the same kernel with the left-right reflection of the board decided per row:
//                     shogi's rules are symmetric under (rank, file) -> (rank, 8 - file), so a reflected row reads mask bit
//                     r * 9 + (8 - c) where the plain one reads r * 9 + c, and its policy target goes through
//                     sl_mirror_action (square reflected, E<->W / NE<->NW / SE<->SW, the two knight jumps swapped, drops
//                     kept).  Value and score do not change.  mode 1 reflects every row, mode 2 the rows whose draw
//                     h(seed, epoch, idx[b]) has its top bit set (include/keisei_amd.h states the draw).  The <false>
//                     instance, which ka_sl_gather launches, contains none of this.
// All are memory-bound copies; nothing in them is tuned further.
#include "common.h"
#include "sl_packed.h"

#include <limits.h>

namespace {

__global__ __launch_bounds__(kPkThreads) void sl_pack_kernel(const uint32_t* __restrict__ records,
                                                             const long long* __restrict__ src_rows, int n,
                                                             uint32_t* __restrict__ packed, int* __restrict__ flags) {
    __shared__ uint32_t s_row[kPkWords];
    __shared__ int s_bad[kPkWaves];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (i >= n) return;
    const long long r = src_rows ? src_rows[i] : (long long)i;
    const uint32_t* src = records + (size_t)r * kPkRowWords;
    const bool bad = sl_pack_channels(src, s_row, lane, wave);
    if (lane == 0) s_bad[wave] = bad;
    bool bad_target = false;
    if (tid == 0) {
        const uint32_t* t = src + kPkObsWords;
        const uint32_t pol_lo = t[0], pol_hi = t[1], val_lo = t[2], val_hi = t[3];
        bad_target = pol_hi != 0u || pol_lo >= kPkActions || val_hi != 0u || val_lo > 2u;
        s_row[kPkPolicyAt + 0] = pol_lo;
        s_row[kPkPolicyAt + 1] = val_lo;
        s_row[kPkPolicyAt + 2] = t[4];
        s_row[kPkPolicyAt + 3] = 0u;
    }
    __syncthreads();
    if (tid < kPkWords) packed[(size_t)i * kPkWords + tid] = s_row[tid];
    if (tid == 0) {
        bool unpackable = false;
        for (int w = 0; w < kPkWaves; ++w) unpackable |= s_bad[w] != 0;
        if (unpackable) { atomicAdd(flags + 0, 1); atomicMin(flags + 1, i); }
        if (bad_target) { atomicAdd(flags + 2, 1); atomicMin(flags + 3, i); }
    }
}

constexpr unsigned long long kSaltMirror = 0x6D6972726F72ull;     // "mirror"

// The reflected action of a spatial action index square * 139 + slot (keisei_amd/shogi_gym.py, _DIRS clockwise from north):
// slots 0..127 = promote * 64 + dir * 8 + (dist - 1), 128..131 = 128 + 2 * side + promote (knight), 132..138 = drops.
__device__ __forceinline__ uint32_t sl_mirror_action(uint32_t a) {
    const uint32_t sq = a / 139u, slot = a - sq * 139u;
    const uint32_t msq = sq + 8u - 2u * (sq % 9u);
    uint32_t mslot = slot;
    if (slot < 128u) mslot = (slot & 64u) | (((8u - ((slot & 63u) >> 3)) & 7u) << 3) | (slot & 7u);
    else if (slot < 132u) mslot = slot ^ 2u;
    return msq * 139u + mslot;
}

template <bool kAug>
__global__ __launch_bounds__(kPkThreads) void sl_gather_kernel(const uint32_t* __restrict__ packed, long long n,
                                                               const long long* __restrict__ idx, int B,
                                                               uint32_t* __restrict__ obs_out, long long* __restrict__ policy_out,
                                                               long long* __restrict__ value_out, uint32_t* __restrict__ score_out,
                                                               int* __restrict__ flags, int mode, unsigned long long seed,
                                                               unsigned epoch) {
    __shared__ uint32_t s_row[kPkWords];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= B) return;
    const long long r = idx[b];
    const bool inside = r >= 0 && r < n;                           // uniform over the workgroup
    bool reflect = false;                                          // uniform too; a row outside the dataset stays all zero
    if constexpr (kAug) {
        if (inside && mode == 1) reflect = true;
        if (inside && mode == 2)
            reflect = (ka_mix64(seed ^ ka_mix64((((unsigned long long)epoch << 32) | (uint32_t)r) + kSaltMirror)) >> 63) != 0ull;
    }
    if (tid < kPkWords) s_row[tid] = inside ? packed[(size_t)r * kPkWords + tid] : 0u;
    __syncthreads();
    uint2* dst = reinterpret_cast<uint2*>(obs_out + (size_t)b * kPkObsWords);
    for (int j = tid; j < kPkObsWords / 2; j += kPkThreads) {
        uint2 out;
        {
            const int e = 2 * j, c = e / kPkSquares;
            int p = e - c * kPkSquares;
            if constexpr (kAug) { if (reflect) p += 8 - 2 * (p % 9); }
            out.x = (s_row[3 * c + (p >> 5)] >> (p & 31)) & 1u ? s_row[kPkValueAt + c] : 0u;
        }
        {
            const int e = 2 * j + 1, c = e / kPkSquares;
            int p = e - c * kPkSquares;
            if constexpr (kAug) { if (reflect) p += 8 - 2 * (p % 9); }
            out.y = (s_row[3 * c + (p >> 5)] >> (p & 31)) & 1u ? s_row[kPkValueAt + c] : 0u;
        }
        dst[j] = out;
    }
    if (tid == 0) {
        if constexpr (kAug) {                                      // (a policy outside the action space is left as stored)
            if (reflect && s_row[kPkPolicyAt + 0] < kPkActions) s_row[kPkPolicyAt + 0] = sl_mirror_action(s_row[kPkPolicyAt + 0]);
        }
        policy_out[b] = (long long)(int)s_row[kPkPolicyAt + 0];
        value_out[b] = (long long)(int)s_row[kPkPolicyAt + 1];
        score_out[b] = s_row[kPkPolicyAt + 2];
        if (!inside) atomicAdd(flags, 1);
    }
}

// The visit rows of a batch (DeviceSLDataset with visit rows): one thread per (batch row, slot).  Visit word k of row idx[b]
// is action | visits << 16, visits 0 = unused; the thread reads the row's eight words for the sum, so w_k is ONE division
// (float)N_k / (float)sum whatever the geometry.  The row is reflected where sl_gather_kernel<true> reflects it: the same
// mode and the same draw.  A used word that names no action counts in the flag word and is handed on as stored.
constexpr int kVisitSlots = 8;

__global__ __launch_bounds__(kPkThreads) void sl_gather_visits_kernel(const uint32_t* __restrict__ visits, long long n,
                                                                      const long long* __restrict__ idx, int B, int mode,
                                                                      unsigned long long seed, unsigned epoch,
                                                                      int* __restrict__ actions_out,
                                                                      float* __restrict__ weights_out, int* __restrict__ flags) {
    const int t = blockIdx.x * kPkThreads + threadIdx.x;
    const int b = t / kVisitSlots, k = t - b * kVisitSlots;
    if (b >= B) return;
    const long long r = idx[b];
    int action = -1;
    float weight = 0.f;
    if (r >= 0 && r < n) {
        const uint32_t* row = visits + (size_t)r * kVisitSlots;
        uint32_t total = 0u;
        for (int j = 0; j < kVisitSlots; ++j) total += row[j] >> 16;
        const uint32_t word = row[k], count = word >> 16;
        if (count != 0u) {
            uint32_t a = word & 0xffffu;
            bool reflect = mode == 1;
            if (mode == 2)
                reflect = (ka_mix64(seed ^ ka_mix64((((unsigned long long)epoch << 32) | (uint32_t)r) + kSaltMirror)) >> 63) != 0ull;
            if (a >= kPkActions) { if (flags) atomicAdd(flags, 1); }
            else if (reflect) a = sl_mirror_action(a);
            action = (int)a;
            weight = (float)count / (float)total;
        }
    }
    actions_out[t] = action;
    weights_out[t] = weight;
}

}  // namespace

extern "C" int ka_sl_packed_words(void) { return kPkWords; }

extern "C" int ka_sl_pack(const void* records, const long long* src_rows, int n, void* packed_out, int* flags, void* stream) {
    KA_REQUIRE(records && packed_out && flags, "sl_pack: null tensor");
    KA_REQUIRE(n > 0, "sl_pack: n %d", n);
    KA_REQUIRE((reinterpret_cast<uintptr_t>(records) & 3) == 0 && (reinterpret_cast<uintptr_t>(packed_out) & 3) == 0,
               "sl_pack: the records and the packed rows must be 4-byte aligned");
    hipLaunchKernelGGL(sl_pack_kernel, dim3(n), dim3(kPkThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint32_t*>(records), src_rows, n, static_cast<uint32_t*>(packed_out), flags);
    return ka_check_launch("sl_pack");
}

extern "C" int ka_sl_gather(const void* packed, long long n, const long long* idx, int B, float* obs_out,
                            long long* policy_out, long long* value_out, float* score_out, int* flags, void* stream) {
    KA_REQUIRE(idx && obs_out && policy_out && value_out && score_out && flags, "sl_gather: null tensor");
    KA_REQUIRE(n >= 0 && (packed || n == 0), "sl_gather: n %lld without a dataset", n);
    KA_REQUIRE(B > 0, "sl_gather: B %d", B);
    KA_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 3) == 0 && (reinterpret_cast<uintptr_t>(obs_out) & 7) == 0,
               "sl_gather: the packed rows must be 4-byte aligned and the observations 8-byte aligned");
    hipLaunchKernelGGL(sl_gather_kernel<false>, dim3(B), dim3(kPkThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint32_t*>(packed), n, idx, B, reinterpret_cast<uint32_t*>(obs_out), policy_out,
                       value_out, reinterpret_cast<uint32_t*>(score_out), flags, 0, 0ull, 0u);
    return ka_check_launch("sl_gather");
}

extern "C" int ka_sl_gather_aug(const void* packed, long long n, const long long* idx, int B, float* obs_out,
                                long long* policy_out, long long* value_out, float* score_out, int* flags, int mode,
                                long long seed, int epoch, void* stream) {
    KA_REQUIRE(mode >= 0 && mode <= 2, "sl_gather_aug: mode %d (0 plain, 1 every row reflected, 2 drawn per row)", mode);
    KA_REQUIRE(epoch >= 0, "sl_gather_aug: epoch %d", epoch);
    if (mode == 0) return ka_sl_gather(packed, n, idx, B, obs_out, policy_out, value_out, score_out, flags, stream);
    KA_REQUIRE(idx && obs_out && policy_out && value_out && score_out && flags, "sl_gather_aug: null tensor");
    KA_REQUIRE(n >= 0 && (packed || n == 0), "sl_gather_aug: n %lld without a dataset", n);
    KA_REQUIRE(B > 0, "sl_gather_aug: B %d", B);
    KA_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 3) == 0 && (reinterpret_cast<uintptr_t>(obs_out) & 7) == 0,
               "sl_gather_aug: the packed rows must be 4-byte aligned and the observations 8-byte aligned");
    hipLaunchKernelGGL(sl_gather_kernel<true>, dim3(B), dim3(kPkThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint32_t*>(packed), n, idx, B, reinterpret_cast<uint32_t*>(obs_out), policy_out,
                       value_out, reinterpret_cast<uint32_t*>(score_out), flags, mode, (unsigned long long)seed,
                       (unsigned)epoch);
    return ka_check_launch("sl_gather_aug");
}

extern "C" int ka_sl_gather_visits(const void* visits, long long n, const long long* idx, int B, int mode, long long seed,
                                   int epoch, int* actions_out, float* weights_out, int* flags, void* stream) {
    KA_REQUIRE(idx && actions_out && weights_out, "sl_gather_visits: null tensor");
    KA_REQUIRE(n >= 0 && (visits || n == 0), "sl_gather_visits: n %lld without visit rows", n);
    KA_REQUIRE(B > 0 && (long long)B * kVisitSlots < (1ll << 31), "sl_gather_visits: B %d", B);
    KA_REQUIRE(mode >= 0 && mode <= 2, "sl_gather_visits: mode %d (0 plain, 1 every row reflected, 2 drawn per row)", mode);
    KA_REQUIRE(epoch >= 0, "sl_gather_visits: epoch %d", epoch);
    KA_REQUIRE((reinterpret_cast<uintptr_t>(visits) & 3) == 0, "sl_gather_visits: the visit rows must be 4-byte aligned");
    const int threads = B * kVisitSlots;
    hipLaunchKernelGGL(sl_gather_visits_kernel, dim3((threads + kPkThreads - 1) / kPkThreads), dim3(kPkThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint32_t*>(visits), n, idx, B, mode,
                       (unsigned long long)seed, (unsigned)epoch, actions_out, weights_out, flags);
    return ka_check_launch("sl_gather_visits");
}
