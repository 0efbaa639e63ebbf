// Sampling controls in the device ply: the play sampler (loss.hip, ka_policy_sample_play) with a temperature, a top-k cut
// and an opening schedule per model.  The reference's showcase plays at SAMPLING_TEMPERATURE = 0.5 (showcase/runner.py:52,
// :155-163); evaluation wants exploratory opening plies and sharp or greedy play behind them; a league wants sharper or more
// diverse opponents.  The logit row lives for one ply in a workspace on the device, so the controls are a kernel in the ply.
//
// One workgroup per row, the logit row and its mask staged once in LDS, as in the play sampler.  Row m of the controls table
// (device memory, read on every launch: a new table applies from the next ply of a captured graph) belongs to model m:
//   word 0 fp32 temperature   1 fp32 opening_temperature   2 int32 opening_plies   3 int32 top_k
// With p the game ply of the row (the u32 the caller points at; no pointer = "infinite"):
//   T = p < opening_plies ? opening_temperature : temperature
//   S = every legal action when top_k == 0 or n_legal <= top_k, else the top_k legal actions that come first in the order
//       "raw logit descending, equal logits by lower action" (the candidate order of ka_policy_insight)
//   T == 0: the first action of that order, probability 1
//   T > 0:  q_j ~ exp((z_j - max_S z) / T) over S, drawn by inverse CDF over S in ascending action order with the play
//           sampler's uniform; log q as Categorical.log_prob clamps it
// A table row with top_k outside [0, 64] or a negative or non-finite temperature is read as the neutral row (T = 1, no cut).
//
// The neutral row is the play sampler to the bit: 1 / T == 1.0f makes the multiply exact, the maximum over S is the maximum
// over the legal actions (the first action of the order is always in S), and the normaliser, the chunk prefix and the walk
// keep the play sampler's order of additions.
//
// The cut: top_k rounds of a block arg-max.  Round r takes the first legal action behind round r - 1's winner in the order,
// so nothing is sorted and nothing in the row is changed; the last winner is the threshold of S.  A round walks the set bits
// of a packed copy of the mask (built by wave ballots while the row is staged), not the actions: a position has tens of
// legal moves, so most threads find no bit and a round is little more than its reduction.  Exact under the tie rule, at
// most 64 rounds, and the usual cuts are a handful of rounds; a bisection over the float's integer image costs 32 counting
// rounds at any top_k plus a second search for the tie.
#include "common.h"

#include <climits>

namespace {

constexpr int kScThreads = 256, kScWaves = kScThreads / 64;
constexpr int kScMaxTop = 64;

struct CtlArgs {
    const void* logits; int logits_bf16; const uint8_t* legal; int legal_words;
    const long long* seed_dev; const int* model_of; int K; const uint32_t* ctl; const uint8_t* plies; int ply_stride;
    long long* actions; float* logp; int* nlegal; int* flags; int A;
};

__device__ __forceinline__ float sc_reduce(float v, float* red, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(v, o); v = is_max ? fmaxf(v, t) : v + t; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < kScWaves; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

// (v, i) comes before (bv, bi) in the candidate order: greater logit, equal logits by lower action (a NaN never does)
__device__ __forceinline__ bool sc_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(kScThreads) void policy_sample_ctl_kernel(CtlArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    uint8_t* msk = reinterpret_cast<uint8_t*>(smem + ((size_t)a.A * 4 + 15) / 16 * 16);
    uint32_t* bits = reinterpret_cast<uint32_t*>(msk + ((size_t)a.A + 15) / 16 * 16);      // the mask again, packed: the rounds walk set bits
    __shared__ float red[kScWaves];
    __shared__ int red_i[kScWaves];
    __shared__ float wave_tot[kScWaves];
    __shared__ int s_first, s_last, s_lo;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = a.A;
    int lo = A;                                                // this thread's lowest legal action
    const uint8_t* lm = a.legal + (size_t)b * A;
    const uint32_t* lw = reinterpret_cast<const uint32_t*>(a.legal) + (size_t)b * a.legal_words;
    float mx = -INFINITY, nlegal = 0.f;
    int nan_seen = 0;
    for (int j = tid; j < A; j += kScThreads) {
        const float v = a.logits_bf16 ? bf2f(static_cast<const uint16_t*>(a.logits)[(size_t)b * A + j])
                                      : static_cast<const float*>(a.logits)[(size_t)b * A + j];
        const uint8_t k = a.legal_words ? (uint8_t)((lw[j >> 5] >> (j & 31)) & 1u) : lm[j];
        row[j] = v; msk[j] = k;
        const unsigned long long bal = __ballot(k != 0);       // a wave stages 64 consecutive actions: two mask words
        if (lane == 0) { bits[j >> 5] = (uint32_t)bal; bits[(j >> 5) + 1] = (uint32_t)(bal >> 32); }
        nan_seen |= (v != v);
        if (k) { mx = fmaxf(mx, v); nlegal += 1.f; }
        if (k && j < lo) lo = j;
    }
    const bool mine = lo < A;                                  // this thread's stride holds a legal action
    if (tid == 0) { s_first = kScThreads; s_last = -1; s_lo = A; }
    mx = sc_reduce(mx, red, true);
    nlegal = sc_reduce(nlegal, red, false);
    const float nanf_ = sc_reduce((float)nan_seen, red, false);
    const int m = a.model_of[b];
    const bool seated = m >= 0 && m < a.K;                     // (uniform over the workgroup, as every branch below)

    // the row's controls
    float T = 1.f;
    int top_k = 0;
    if (seated) {
        const uint32_t* c = a.ctl + (size_t)m * 4;
        const float t_late = __uint_as_float(c[0]), t_open = __uint_as_float(c[1]);
        const int opening = (int)c[2], k = (int)c[3];
        const bool ok = t_late >= 0.f && t_late <= 3.0e38f && t_open >= 0.f && t_open <= 3.0e38f && k >= 0 && k <= kScMaxTop;
        if (ok) {
            const uint32_t p = a.plies ? *reinterpret_cast<const uint32_t*>(a.plies + (size_t)b * a.ply_stride) : UINT_MAX;
            T = (opening > 0 && p < (uint32_t)opening) ? t_open : t_late;
            top_k = k;
        }
    }
    const bool greedy = T == 0.f;
    const bool cut = top_k > 0 && nlegal > (float)top_k;
    const int rounds = !seated ? 0 : greedy ? 1 : cut ? top_k : 0;

    // the first `rounds` actions of the candidate order: round r takes the first one behind round r - 1's winner
    const int words = (A + 63) / 64 * 2;
    float tv = INFINITY;
    int ti = -1, first_i = INT_MAX;
    for (int r = 0; r < rounds; ++r) {
        float bv = -INFINITY;
        int bi = INT_MAX;
        for (int w = tid; w < words; w += kScThreads) {
            uint32_t mw = bits[w];
            while (mw) {
                const int j = (w << 5) + __builtin_ctz(mw);
                mw &= mw - 1u;
                const float v = row[j];
                if (sc_before(tv, ti, v, j) && sc_before(v, j, bv, bi)) { bv = v; bi = j; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (sc_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        __syncthreads();
        if (lane == 0) { red[wave] = bv; red_i[wave] = bi; }
        __syncthreads();
        bv = red[0]; bi = red_i[0];
        for (int w = 1; w < kScWaves; ++w)
            if (sc_before(red[w], red_i[w], bv, bi)) { bv = red[w]; bi = red_i[w]; }
        if (bi == INT_MAX) break;                              // nothing behind the last winner (NaN logits only): it stays the threshold
        tv = bv; ti = bi;
        if (r == 0) first_i = bi;
    }

    if (!seated || (greedy && nlegal > 0.f)) {
        // an unseated row takes its first legal action (log-prob 0); a greedy row the first action of the order (probability 1)
        if (mine) atomicMin(&s_lo, lo);
        __syncthreads();
        if (tid == 0) {
            if (nanf_ > 0.f) atomicOr(&a.flags[0], 1);
            if (nlegal == 0.f) atomicOr(&a.flags[1], 1);
            a.nlegal[b] = (int)nlegal;
            if (!seated) {
                a.actions[b] = s_lo < A ? s_lo : 0;
                a.logp[b] = 0.f;
            } else {
                a.actions[b] = first_i != INT_MAX ? first_i : s_lo;
                a.logp[b] = logf(1.f - 1.1920929e-7f);
            }
        }
        return;
    }

    // T > 0 from here on (a greedy row without a legal action ends below as every such row does)
    const float inv_t = greedy ? 1.f : fminf(1.f / T, 3.0e38f);
    const bool limited = cut && ti >= 0;                       // S = the legal actions not behind the threshold (tv, ti)
    auto in_s = [&](int j) -> bool { return msk[j] && (!limited || !sc_before(tv, ti, row[j], j)); };
    float s = 0.f;
    for (int j = tid; j < A; j += kScThreads)
        if (in_s(j)) s += expf((row[j] - mx) * inv_t);
    s = sc_reduce(s, red, false);                              // the normaliser of the masked-softmax path (same order)
    // contiguous chunk per thread, inclusive prefix over the threads
    const int chunk = (A + kScThreads - 1) / kScThreads, j0 = tid * chunk, j1 = min(j0 + chunk, A);
    float local = 0.f;
    for (int j = j0; j < j1; ++j) if (in_s(j)) local += expf((row[j] - mx) * inv_t);
    float incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    float base = 0.f, total = 0.f;
    for (int w = 0; w < kScWaves; ++w) { if (w < wave) base += wave_tot[w]; total += wave_tot[w]; }
    incl += base;
    const unsigned long long seed = (unsigned long long)*a.seed_dev;
    // the play sampler's draw (loss.hip): the same (seed, row) gives the same uniform
    const unsigned long long h = ka_mix64(seed ^ ka_mix64((unsigned long long)b + 0x5851F42D4C957F2Dull));
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);   // 24 bits: [0, 1)
    const float target = u * total;
    if (local > 0.f) {                                         // (as the play sampler: a chunk whose weights all underflow is no chunk of S)
        if (incl > target) atomicMin(&s_first, tid);
        atomicMax(&s_last, tid);
    }
    __syncthreads();
    const int winner = s_first < kScThreads ? s_first : s_last;           // (rounding can leave target >= total: last chunk of S)
    if (tid == 0) {
        if (nanf_ > 0.f) atomicOr(&a.flags[0], 1);
        if (nlegal == 0.f) { atomicOr(&a.flags[1], 1); a.actions[b] = 0; a.logp[b] = 0.f; }
        a.nlegal[b] = (int)nlegal;
    }
    if (tid == winner) {
        float run = incl - local;
        int pick = -1, last = -1;
        for (int j = j0; j < j1; ++j) {
            if (!in_s(j)) continue;
            last = j;
            run += expf((row[j] - mx) * inv_t);
            if (run > target) { pick = j; break; }
        }
        if (pick < 0) pick = last;
        a.actions[b] = pick;
        // Categorical(probs).log_prob = log(clamp(q, eps, 1 - eps)), eps = FLT_EPSILON
        const float q = expf((row[pick] - mx) * inv_t) * (1.f / s);
        a.logp[b] = logf(fminf(fmaxf(q, 1.1920929e-7f), 1.f - 1.1920929e-7f));
    }
}

}  // namespace

extern "C" int ka_policy_sample_ctl(const void* logits, int logits_bf16, const void* legal, int legal_words,
                                    const long long* seed_dev, const int* model_of, int K, const void* ctl, const void* plies,
                                    int ply_stride, long long* actions, float* logp, int* nlegal, int* flags, int B, int A,
                                    void* stream) {
    KA_REQUIRE(logits && legal && seed_dev && model_of && ctl && actions && logp && nlegal && flags && B > 0 && A > 0,
               "policy_sample_ctl: null tensor");
    KA_REQUIRE(legal_words == 0 || legal_words == (A + 31) / 32, "policy_sample_ctl: packed mask rows must hold %d words", (A + 31) / 32);
    const size_t lds = ((size_t)A * 4 + 15) / 16 * 16 + ((size_t)A + 15) / 16 * 16 + ((size_t)A + 63) / 64 * 8;
    KA_REQUIRE(lds <= 64 * 1024, "policy_sample_ctl: action space %d too large for the LDS row", A);
    KA_REQUIRE(K >= 1, "policy_sample_ctl: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE(!plies || ply_stride >= 4, "policy_sample_ctl: ply_stride must be at least 4 bytes, got %d", ply_stride);
    KA_REQUIRE((uintptr_t)ctl % 4 == 0 && (!plies || ((uintptr_t)plies % 4 == 0 && ply_stride % 4 == 0)),
               "policy_sample_ctl: the controls table and the game plies are read as aligned 32-bit words");
    CtlArgs a{logits, logits_bf16, static_cast<const uint8_t*>(legal), legal_words, seed_dev, model_of, K,
              static_cast<const uint32_t*>(ctl), static_cast<const uint8_t*>(plies), ply_stride, actions, logp, nlegal, flags, A};
    hipLaunchKernelGGL(policy_sample_ctl_kernel, dim3(B), dim3(kScThreads), lds, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_sample_ctl");
}
