// A row of policy logits under a legal mask, stated once: the candidate order, one round of "the first action behind the
// previous winner", the staged row with its maximum and counts, the normaliser, the inverse-CDF draw with its uniform, and
// the endings of a row that is not drawn.  The loss, the masked softmax and the samplers (csrc/loss.hip), the sampling
// controls (csrc/sampling.hip), the policy insight (csrc/insight.hip) and the fork of the lookahead and the tree search
// (csrc/lookahead.hip) promise to agree to the bit -- the neutral controls row is the play sampler, the controls cut and the
// fork take the insight's candidates, one (seed, row) gives one uniform -- and they do because each of these is one body.
// The float sums go through common.h's ka_block_sum / ka_block_max.
//
// Two LDS layouts are served, not unified.  The dynamic one (loss.hip, sampling.hip): an fp32 row and a byte mask over a
// run-time A, and for the controls a packed copy of the mask.  The static one (insight.hip, lookahead.hip): a row over the
// spatial action space of which only the legal positions are ever written or read, and the packed mask.
#pragma once
#include "common.h"

#include <climits>

// ---- the dynamic layout: byte offsets of the pieces, and what the launchers check (host side)
__host__ __device__ constexpr size_t policy_row_bytes(int A) { return ((size_t)A * 4 + 15) / 16 * 16; }     // the fp32 row
__host__ __device__ constexpr size_t policy_mask_bytes(int A) { return ((size_t)A + 15) / 16 * 16; }        // the byte mask behind it
__host__ __device__ constexpr size_t policy_bits_bytes(int A) { return ((size_t)A + 63) / 64 * 8; }         // the packed copy: two words per 64 actions
#define KA_REQUIRE_MASK_ROW(who, A, legal_words)                                                                   \
    KA_REQUIRE((legal_words) == 0 || (legal_words) == ((A) + 31) / 32, who ": packed mask rows must hold %d words", ((A) + 31) / 32)
#define KA_REQUIRE_ROW_LDS(who, lds, A) KA_REQUIRE((lds) <= 64 * 1024, who ": action space %d too large for the LDS row", (A))

// logit i of a tensor of fp32 or bf16 logits
__device__ __forceinline__ float policy_logit(const void* logits, int bf16, size_t i) {
    return bf16 ? bf2f(static_cast<const uint16_t*>(logits)[i]) : static_cast<const float*>(logits)[i];
}
// action j of the mask row: bool bytes at lm (legal_words == 0) or packed words at lw, bit j & 31 of word j >> 5
__device__ __forceinline__ uint8_t policy_legal(const uint8_t* lm, const uint32_t* lw, int legal_words, int j) {
    return legal_words ? (uint8_t)((lw[j >> 5] >> (j & 31)) & 1u) : lm[j];
}

// ---- the candidate order
// (v, i) comes before (bv, bi): greater logit, equal logits by lower action (a NaN comes before nothing and behind nothing)
__device__ __forceinline__ bool policy_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// f(j) for every set bit j of this thread's words of a packed mask (words t, t + THREADS, ...), in ascending j
template <int THREADS, class F>
__device__ __forceinline__ void policy_for_legal(const uint32_t* msk, int words, F f) {
    for (int w = threadIdx.x; w < words; w += THREADS) {
        uint32_t m = msk[w];
        while (m) {
            f((w << 5) + __builtin_ctz(m));
            m &= m - 1u;
        }
    }
}

// One round: the first legal action behind (prev_v, prev_i) in the order -- (INFINITY, -1) is in front of all -- or INT_MAX
// when there is none; *best_v is its logit.  Uniform over the workgroup.  A NaN is never taken; a legal -inf only with
// kAllowNegInf (the controls' cut counts it, the insight and the fork do not).  The loop around the rounds is the caller's.
template <int THREADS, bool kAllowNegInf>
__device__ __forceinline__ int policy_next(const float* row, const uint32_t* msk, int words, float prev_v, int prev_i,
                                           float* red, int* red_i, float* best_v) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    policy_for_legal<THREADS>(msk, words, [&](int j) {
        const float v = row[j];
        if ((kAllowNegInf || v > -INFINITY) && policy_before(prev_v, prev_i, v, j) && policy_before(v, j, bv, bi)) { bv = v; bi = j; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (policy_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = bv; red_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bv = red[0]; bi = red_i[0];
    for (int w = 1; w < THREADS / 64; ++w)
        if (policy_before(red[w], red_i[w], bv, bi)) { bv = red[w]; bi = red_i[w]; }
    *best_v = bv;
    return bi;
}

// ---- the staged row
// What staging finds: the maximum over the legal logits, the number of legal actions and of NaN logits seen (> 0 = some),
// and the thread's own lowest legal action (A = none).  Staging leaves the thread's share in it; reduce() makes the first
// three the row's.
struct PolicyRowHead {
    float mx, nlegal, nan;
    int lo;
    template <int THREADS> __device__ __forceinline__ void reduce(float* red) {
        mx = ka_block_max<THREADS>(mx, red);
        nlegal = ka_block_sum<THREADS>(nlegal, red);
        nan = ka_block_sum<THREADS>(nan, red);
    }
};

// The dynamic layout: row b of the logits (fp32 or bf16) and of the mask (bool or packed) into row[] and msk[], action j by
// thread j % THREADS.  kLowest keeps the thread's lowest legal action; kPack builds the packed copy in bits[] by wave
// ballots (a wave stages 64 consecutive actions: two mask words).  A NaN counts whether or not its action is legal.
template <int THREADS, bool kLowest, bool kPack>
__device__ __forceinline__ PolicyRowHead policy_stage(const void* logits, int bf16, const uint8_t* legal, int legal_words, int b,
                                                      int A, float* row, uint8_t* msk, uint32_t* bits) {
    const uint8_t* lm = legal + (size_t)b * A;
    const uint32_t* lw = reinterpret_cast<const uint32_t*>(legal) + (size_t)b * legal_words;
    float mx = -INFINITY, nlegal = 0.f;
    int nan_seen = 0, lo = A;
    for (int j = threadIdx.x; j < A; j += THREADS) {
        const float v = policy_logit(logits, bf16, (size_t)b * A + j);
        const uint8_t k = policy_legal(lm, lw, legal_words, j);
        row[j] = v; msk[j] = k;
        if constexpr (kPack) {
            const unsigned long long bal = __ballot(k != 0);
            if ((threadIdx.x & 63) == 0) { bits[j >> 5] = (uint32_t)bal; bits[(j >> 5) + 1] = (uint32_t)(bal >> 32); }
        }
        nan_seen |= (v != v);
        if (k) { mx = fmaxf(mx, v); nlegal += 1.f; }
        if constexpr (kLowest) { if (k && j < lo) lo = j; }
    }
    return PolicyRowHead{mx, nlegal, (float)nan_seen, lo};
}

// The static layout: the logits behind the set bits of msk[] (filled by the caller; a thread reads back the words it wrote
// itself) from memory into row[] at the action's index.  A NaN is passed over by the maximum; lo is not kept (INT_MAX).
template <int THREADS>
__device__ __forceinline__ PolicyRowHead policy_stage_legal(const void* logits, int bf16, size_t first, const uint32_t* msk,
                                                            int words, float* row) {
    float mx = -INFINITY, nlegal = 0.f;
    int nan_seen = 0;
    policy_for_legal<THREADS>(msk, words, [&](int j) {
        const float v = policy_logit(logits, bf16, first + j);
        row[j] = v;
        nan_seen |= (v != v);
        mx = fmaxf(mx, v);
        nlegal += 1.f;
    });
    return PolicyRowHead{mx, nlegal, (float)nan_seen, INT_MAX};
}

// The normaliser of the dynamic layout: the sum of weight(j) over the actions j with in_s(j), thread t adding t, t + THREADS,
// ... in turn.  The weight is the caller's expression -- expf(row[j] - mx), or the controls' expf((row[j] - mx) * inv_t) --
// so a kernel without a temperature has no multiply.
template <int THREADS, class InS, class Weight>
__device__ __forceinline__ float policy_normaliser(int A, InS in_s, Weight weight, float* red) {
    float s = 0.f;
    for (int j = threadIdx.x; j < A; j += THREADS)
        if (in_s(j)) s += weight(j);
    return ka_block_sum<THREADS>(s, red);
}

// ---- the draw and the endings
// The uniform of row b under a seed: 24 bits, [0, 1)
__device__ __forceinline__ float policy_uniform(unsigned long long seed, int b) {
    const unsigned long long h = ka_mix64(seed ^ ka_mix64((unsigned long long)b + 0x5851F42D4C957F2Dull));
    return (float)(h >> 40) * (1.0f / 16777216.0f);
}

// what the draw and the endings keep in LDS; reset() by every thread, with a barrier (a reduce) before the first use
template <int THREADS> struct PolicyDrawLds {
    float wave_tot[THREADS / 64];
    int first, last, lo;
    __device__ __forceinline__ void reset(int A) {
        if (threadIdx.x == 0) { first = THREADS; last = -1; lo = A; }
    }
};

// Thread 0's part of every ending: flags[0] |= a NaN among the logits, flags[1] |= a row without a legal action (its action
// is 0, its log-prob 0), and the number of legal actions.
__device__ __forceinline__ void policy_report(const PolicyRowHead& h, int* flags, int* nlegal, long long* action, float* logp) {
    if (h.nan > 0.f) atomicOr(&flags[0], 1);
    if (h.nlegal == 0.f) { atomicOr(&flags[1], 1); *action = 0; *logp = 0.f; }
    *nlegal = (int)h.nlegal;
}

// the lowest legal action of the row from every thread's own (A = none); every thread calls it
template <int THREADS>
__device__ __forceinline__ int policy_lowest(const PolicyRowHead& h, int A, PolicyDrawLds<THREADS>& d) {
    if (h.lo < A) atomicMin(&d.lo, h.lo);
    __syncthreads();
    return d.lo;
}

// The ending of an unseated row (the reference's legal_masks.argmax(-1) for idle partitions): its first legal action, log-prob 0
template <int THREADS>
__device__ __forceinline__ void policy_end_unseated(const PolicyRowHead& h, int A, PolicyDrawLds<THREADS>& d, int* flags, int* nlegal,
                                                    long long* action, float* logp) {
    const int first = policy_lowest(h, A, d);
    if (threadIdx.x == 0) {
        policy_report(h, flags, nlegal, action, logp);
        *action = first < A ? first : 0;
        *logp = 0.f;
    }
}

// One action of the row by inverse CDF over S = {j : in_s(j)} in ascending action order, and its log-probability as
// Categorical.log_prob clamps it (katago_ppo.py:603-605: log(clamp(p, eps, 1 - eps)), eps = FLT_EPSILON, so an action more
// than ~88 nats below the maximum gives log(eps), not -inf).  A contiguous chunk per thread, an inclusive prefix over the
// threads, the first chunk whose running total passes u * total is walked by its thread; rounding can leave u * total >=
// total, then the last chunk of S is.  A chunk whose weights all underflow is no chunk of S.  s is policy_normaliser's sum
// over the same S and weight.  A row in which no chunk has weight writes nothing.
template <int THREADS, class InS, class Weight>
__device__ __forceinline__ void policy_draw(int A, int b, unsigned long long seed, float s, InS in_s, Weight weight,
                                            PolicyDrawLds<THREADS>& d, long long* action, float* logp) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (A + THREADS - 1) / THREADS, j0 = tid * chunk, j1 = min(j0 + chunk, A);
    float local = 0.f;
    for (int j = j0; j < j1; ++j) if (in_s(j)) local += weight(j);
    float incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (lane == 63) d.wave_tot[wave] = incl;
    __syncthreads();
    float base = 0.f, total = 0.f;
    for (int w = 0; w < THREADS / 64; ++w) { if (w < wave) base += d.wave_tot[w]; total += d.wave_tot[w]; }
    incl += base;
    const float target = policy_uniform(seed, b) * total;
    if (local > 0.f) {
        if (incl > target) atomicMin(&d.first, tid);
        atomicMax(&d.last, tid);
    }
    __syncthreads();
    const int winner = d.first < THREADS ? d.first : d.last;
    if (tid == winner) {
        float run = incl - local;
        int pick = -1, last = -1;
        for (int j = j0; j < j1; ++j) {
            if (!in_s(j)) continue;
            last = j;
            run += weight(j);
            if (run > target) { pick = j; break; }
        }
        if (pick < 0) pick = last;
        *action = pick;
        const float p = weight(pick) * (1.f / s);
        *logp = logf(fminf(fmaxf(p, 1.1920929e-7f), 1.f - 1.1920929e-7f));
    }
}
