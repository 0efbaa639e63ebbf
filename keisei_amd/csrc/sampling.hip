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
//
// The candidate order, the round, the staged row, the draw and its uniform are csrc/policy_row.h's: the bodies the play
// sampler, the insight and the fork run, which is what keeps the promises above.
#include "policy_row.h"

namespace {

constexpr int kScThreads = 256, kScWaves = kScThreads / 64;
constexpr int kScMaxTop = 64;

struct CtlArgs {
    const void* logits; int logits_bf16; const uint8_t* legal; int legal_words;
    const long long* seed_dev; const int* model_of; int K; const uint32_t* ctl; const uint8_t* plies; int ply_stride;
    long long* actions; float* logp; int* nlegal; int* flags; int A;
};

__global__ __launch_bounds__(kScThreads) void policy_sample_ctl_kernel(CtlArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    uint8_t* msk = reinterpret_cast<uint8_t*>(smem + policy_row_bytes(a.A));
    uint32_t* bits = reinterpret_cast<uint32_t*>(msk + policy_mask_bytes(a.A));          // the mask again, packed: the rounds walk set bits
    __shared__ float red[kScWaves];
    __shared__ int red_i[kScWaves];
    __shared__ PolicyDrawLds<kScThreads> draw;
    const int b = blockIdx.x, tid = threadIdx.x, A = a.A;
    PolicyRowHead h = policy_stage<kScThreads, true, true>(a.logits, a.logits_bf16, a.legal, a.legal_words, b, A, row, msk, bits);
    draw.reset(A);
    h.reduce<kScThreads>(red);
    const float mx = h.mx, nlegal = h.nlegal;
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
        float bv;
        const int bi = policy_next<kScThreads, true>(row, bits, words, tv, ti, red, red_i, &bv);
        if (bi == INT_MAX) break;                              // nothing behind the last winner (NaN logits only): it stays the threshold
        tv = bv; ti = bi;
        if (r == 0) first_i = bi;
    }

    if (!seated) {                                             // its first legal action, log-prob 0
        policy_end_unseated(h, A, draw, a.flags, &a.nlegal[b], &a.actions[b], &a.logp[b]);
        return;
    }
    if (greedy && nlegal > 0.f) {                              // the first action of the order, probability 1
        const int lowest = policy_lowest(h, A, draw);
        if (tid == 0) {
            policy_report(h, a.flags, &a.nlegal[b], &a.actions[b], &a.logp[b]);
            a.actions[b] = first_i != INT_MAX ? first_i : lowest;
            a.logp[b] = logf(1.f - 1.1920929e-7f);
        }
        return;
    }

    // T > 0 from here on (a greedy row without a legal action ends below as every such row does)
    const float inv_t = greedy ? 1.f : fminf(1.f / T, 3.0e38f);
    const bool limited = cut && ti >= 0;                       // S = the legal actions not behind the threshold (tv, ti)
    const auto in_s = [&](int j) -> bool { return msk[j] && (!limited || !policy_before(tv, ti, row[j], j)); };
    const auto weight = [&](int j) { return expf((row[j] - mx) * inv_t); };
    const float s = policy_normaliser<kScThreads>(A, in_s, weight, red);
    policy_draw(A, b, (unsigned long long)*a.seed_dev, s, in_s, weight, draw, &a.actions[b], &a.logp[b]);
    if (tid == 0) policy_report(h, a.flags, &a.nlegal[b], &a.actions[b], &a.logp[b]);
}

}  // namespace

extern "C" int ka_policy_sample_ctl(const void* logits, int logits_bf16, const void* legal, int legal_words,
                                    const long long* seed_dev, const int* model_of, int K, const void* ctl, const void* plies,
                                    int ply_stride, long long* actions, float* logp, int* nlegal, int* flags, int B, int A,
                                    void* stream) {
    KA_REQUIRE(logits && legal && seed_dev && model_of && ctl && actions && logp && nlegal && flags && B > 0 && A > 0,
               "policy_sample_ctl: null tensor");
    KA_REQUIRE_MASK_ROW("policy_sample_ctl", A, legal_words);
    const size_t lds = policy_row_bytes(A) + policy_mask_bytes(A) + policy_bits_bytes(A);
    KA_REQUIRE_ROW_LDS("policy_sample_ctl", lds, A);
    KA_REQUIRE(K >= 1, "policy_sample_ctl: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE(!plies || ply_stride >= 4, "policy_sample_ctl: ply_stride must be at least 4 bytes, got %d", ply_stride);
    KA_REQUIRE((uintptr_t)ctl % 4 == 0 && (!plies || ((uintptr_t)plies % 4 == 0 && ply_stride % 4 == 0)),
               "policy_sample_ctl: the controls table and the game plies are read as aligned 32-bit words");
    CtlArgs a{logits, logits_bf16, static_cast<const uint8_t*>(legal), legal_words, seed_dev, model_of, K,
              static_cast<const uint32_t*>(ctl), static_cast<const uint8_t*>(plies), ply_stride, actions, logp, nlegal, flags, A};
    hipLaunchKernelGGL(policy_sample_ctl_kernel, dim3(B), dim3(kScThreads), lds, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_sample_ctl");
}
