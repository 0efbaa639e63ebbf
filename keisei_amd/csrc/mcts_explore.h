// What the two exploration controls of the visit-count search share (csrc/mcts_explore.hip draws the root noise,
// csrc/mcts.hip draws the played move): the table row of a model and the random streams.  The Python restatement is
// keisei_amd/training/mcts_explore.py.
//
// Table: K rows of 4 words, row m for model m:  0 fp32 noise_fraction (epsilon, [0, 1])   1 fp32 noise_alpha ([0.01, 100]
// when epsilon > 0, else not looked at)   2 int32 sample_plies ([0, 65535])   3 reserved, 0.  A row with a word out of range
// (a NaN included) reads as off (0, 0, 0), and so does a model outside [0, K).
//
// Streams.  seed is the int64 at the head of the loop's state array (what the sampler reads this ply).  The stream of env e
// for purpose C is h = ka_mix64(seed ^ ka_mix64(e + C)), draw i of it r_i = ka_mix64(h + i * kKaWeyl), and a uniform in the
// open interval (0, 1) is ((r >> 12) + 0.5) * 2^-52 (exact in fp64).  The purposes, both distinct from the sampler's
// 0x5851F42D4C957F2D:
//   kXpNoise   0x2545F4914F6CDD1D   the Dirichlet draw of ka_mcts_root_noise
//   kXpChoice  0xD1342543DE82EF95   the played move of ka_mcts_advance_explore (draw 0 only)
// Draw indices of the noise stream, for slot k (0..7) and try j (0..15):
//   64 k + 3 j + 0   u0, Box-Muller radius          64 k + 3 j + 1   u1, Box-Muller angle
//   64 k + 3 j + 2   u2, the accept test            64 k + 48        u_b, the boost of alpha < 1
#pragma once
#include "lookahead_record.h"

constexpr unsigned long long kXpNoise = 0x2545F4914F6CDD1Dull, kXpChoice = 0xD1342543DE82EF95ull;
constexpr int kXpStatsWords = 4;                               // noised, sampled, diverged, reserved
constexpr int kXpTries = 16, kXpSlotDraws = 64, kXpBoostDraw = 48;
constexpr int kXpMaxSamplePlies = 65535;

__device__ __forceinline__ unsigned long long xp_stream(unsigned long long seed, int e, unsigned long long purpose) {
    return ka_mix64(seed ^ ka_mix64((unsigned long long)e + purpose));
}
__device__ __forceinline__ unsigned long long xp_draw(unsigned long long h, int i) {
    return ka_mix64(h + (unsigned long long)i * kKaWeyl);
}
__device__ __forceinline__ double xp_uniform(unsigned long long r) {
    return ((double)(r >> 12) + 0.5) * 0x1p-52;
}

// the exploration controls of model m as the kernels read them; off is (0, 0, 0)
__device__ __forceinline__ void xp_controls(const uint32_t* table, int m, int K, float* eps, float* alpha, int* sample_plies) {
    *eps = 0.f; *alpha = 0.f; *sample_plies = 0;
    if (m < 0 || m >= K) return;
    const uint32_t* c = table + (size_t)m * kLaTableWords;
    const float e = __uint_as_float(c[0]), a = __uint_as_float(c[1]);
    const int s = (int)c[2];
    if (!(e >= 0.f && e <= 1.f && (e == 0.f || (a >= 0.01f && a <= 100.f)) && s >= 0 && s <= kXpMaxSamplePlies)) return;
    *eps = e; *alpha = e > 0.f ? a : 0.f; *sample_plies = s;
}
