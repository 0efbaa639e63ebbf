// Exploration for the visit-count search of csrc/mcts.hip: Dirichlet noise in the root priors.  (The other control, the move
// drawn in proportion to the root visits, is a branch of mcts_advance_kernel; the table row and the random streams both read
// are in csrc/mcts_explore.h.)
//
//   ka_mcts_root_noise   between ka_lookahead_fork and ka_mcts_advance(t = 0): for every env whose record 0 is active and
//                        whose model has epsilon > 0, with n = clamp(n_cand, 1, width) candidates of priors p_k:
//                          eta ~ Dirichlet(alpha) over the n candidates, s = p_0 + .. + p_{n-1} in slot order,
//                          p'_k = (1 - epsilon) p_k + epsilon s eta_k, all fp64, rounded once to fp32 into the record.
//                        The candidates' prior mass is kept, so c_puct means the same with noise on and off.  The advance
//                        copies the record's priors into the tree: nothing downstream changes.
//
// The Dirichlet draw, all fp64, from the noise stream of (seed, env) (draw indices: csrc/mcts_explore.h).  Gamma(alpha) of
// slot k by Marsaglia-Tsang: a' = alpha < 1 ? alpha + 1 : alpha, d = a' - 1/3, c = 1 / sqrt(9 d); at most 16 tries, try j
// from draws 64 k + 3 j + {0, 1, 2}: x = sqrt(-2 ln u0) cos(2 pi u1), t = 1 + c x, v = t t t; rejected if v <= 0, accepted if
// ln u2 < 0.5 x x + d - d v + d ln v.  g = d v, or d where all 16 tries rejected; for alpha < 1 times exp(ln(u_b) / alpha)
// with u_b draw 64 k + 48.  eta_k = g_k / sum g (summed in slot order), or 1 / n where the sum is not above 0 or not finite.
//
// Why fp64: there are at most eight values per env and ply, so the latency of the fp64 transcendentals is of no account,
// and the device's and the host's log / cos / exp then differ in the last bits of a double -- far below the distance of any
// accept test from flipping (the restatement reports that distance) and below an fp32 ulp of the result.  This file is
// compiled without fp contraction, so that +, *, / and sqrt are the restatement's to the bit.
//
// One lane per (env, slot), eight lanes per env whatever the width: eight envs per wave, thirty-two per block, no loop over
// slots.  The eight lanes exchange p and g by shuffles and every one adds them in slot order: the order of the fp64 sums is
// part of the contract.  Rows that are inactive, off or of a model outside [0, K) are not written at all.
#include "mcts_explore.h"

#include <climits>

namespace {

constexpr int kXpThreads = 256, kXpLanes = 8;
static_assert(kXpLanes == kLaMaxWidth, "one lane per slot");
static_assert(3 * kXpTries <= kXpBoostDraw && kXpBoostDraw < kXpSlotDraws, "the draws of a slot do not overlap");

struct NoiseArgs {
    uint32_t* rec; int width; const uint32_t* table; const int* model_of; int K; const long long* seed_dev;
    float* raw; double* eta; int* stats; int n;
};

// Gamma(alpha) of slot k from the stream h (Marsaglia-Tsang, at most kXpTries tries)
__device__ double xp_gamma(unsigned long long h, int k, double alpha) {
    const double a1 = alpha < 1.0 ? alpha + 1.0 : alpha;
    const double d = a1 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = d;
    for (int j = 0; j < kXpTries; ++j) {
        const int i = k * kXpSlotDraws + 3 * j;
        const double u0 = xp_uniform(xp_draw(h, i)), u1 = xp_uniform(xp_draw(h, i + 1)), u2 = xp_uniform(xp_draw(h, i + 2));
        const double x = sqrt(-2.0 * log(u0)) * cos(6.283185307179586 * u1);
        const double t = 1.0 + c * x, v = t * t * t;
        if (v <= 0.0) continue;
        if (log(u2) < 0.5 * x * x + d - d * v + d * log(v)) { g = d * v; break; }
    }
    if (alpha < 1.0) g = g * exp(log(xp_uniform(xp_draw(h, k * kXpSlotDraws + kXpBoostDraw))) / alpha);
    return g;
}

__global__ __launch_bounds__(kXpThreads) void mcts_root_noise_kernel(NoiseArgs a) {
    const int idx = blockIdx.x * kXpThreads + threadIdx.x, e = idx / kXpLanes, k = idx % kXpLanes;
    const int lane = threadIdx.x & 63, first = lane & ~(kXpLanes - 1);
    const int width = a.width;
    uint32_t* rec = nullptr;
    bool on = false;
    int n = 0;
    float eps = 0.f, alpha = 0.f;
    if (e < a.n) {
        int sample_plies;
        rec = a.rec + (size_t)e * la_words(width);
        xp_controls(a.table, a.model_of[e], a.K, &eps, &alpha, &sample_plies);
        on = (rec[kLaFlags] & 1u) != 0 && eps > 0.f;
        n = min(max((int)rec[kLaNCand], 1), width);
    }
    const bool mine = on && k < n;
    uint32_t bits = 0u;
    double p = 0.0, g = 0.0;
    if (mine) {
        bits = rec[kLaCand + width + k];
        p = (double)__uint_as_float(bits);
        g = xp_gamma(xp_stream((unsigned long long)*a.seed_dev, e, kXpNoise), k, (double)alpha);
    }
    double s = 0.0, gs = 0.0;                                  // every lane of the wave takes part in the shuffles
    for (int j = 0; j < kXpLanes; ++j) {
        const double pj = __shfl(p, first + j), gj = __shfl(g, first + j);
        if (j < n) { s += pj; gs += gj; }
    }
    if (on && k < width) {
        double eta = 0.0;
        if (mine) {
            eta = gs > 0.0 && gs <= 1.7976931348623157e308 ? g / gs : 1.0 / (double)n;
            const double mixed = (1.0 - (double)eps) * p + (double)eps * s * eta;
            rec[kLaCand + width + k] = __float_as_uint((float)mixed);
        }
        a.raw[(size_t)e * width + k] = __uint_as_float(bits);
        a.eta[(size_t)e * width + k] = eta;
    }
    const int noised = __popcll(__ballot(on && k == 0));
    if (lane == 0 && noised) atomicAdd(&a.stats[0], noised);
}

}  // namespace

extern "C" int ka_mcts_root_noise(void* records, int width, const void* explore_table, const int* model_of, int K,
                                  const long long* seed_dev, float* raw_priors, double* eta, int* explore_stats, int N,
                                  void* stream) {
    KA_REQUIRE(records && explore_table && model_of && seed_dev && raw_priors && eta && explore_stats && N > 0,
               "mcts_root_noise: null tensor");
    KA_REQUIRE(width >= 1 && width <= kLaMaxWidth, "mcts_root_noise: width must lie in [1, %d], got %d", kLaMaxWidth, width);
    KA_REQUIRE(K >= 1, "mcts_root_noise: the exploration table needs at least one row, got K = %d", K);
    KA_REQUIRE((long long)N * kXpLanes <= INT_MAX, "mcts_root_noise: too many envs");
    KA_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)explore_table % 4 == 0 && (uintptr_t)model_of % 4 == 0 &&
               (uintptr_t)seed_dev % 8 == 0 && (uintptr_t)raw_priors % 4 == 0 && (uintptr_t)eta % 8 == 0 &&
               (uintptr_t)explore_stats % 4 == 0,
               "mcts_root_noise: the seed and eta are 8-byte aligned, every other tensor to its element size");
    NoiseArgs a{static_cast<uint32_t*>(records), width, static_cast<const uint32_t*>(explore_table), model_of, K, seed_dev,
                raw_priors, eta, explore_stats, N};
    const long long threads = (long long)N * kXpLanes;
    hipLaunchKernelGGL(mcts_root_noise_kernel, dim3((unsigned)((threads + kXpThreads - 1) / kXpThreads)), dim3(kXpThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mcts_root_noise");
}
