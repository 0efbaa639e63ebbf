// What the value searches of the device ply share: the record of an env, the controls row of a model and the leaf value of
// a forked row.  The lookahead, its reply search and the tree search (csrc/lookahead.hip) and the visit-count search
// (csrc/mcts.hip) read them from here, so that a candidate, a prior and a leaf q mean the same in every one of them.
#pragma once
#include "ply_rows.h"

constexpr int kLaMaxWidth = 8;
constexpr int kLaFlags = 0, kLaSlot = 1, kLaNCand = 2, kLaAction = 3, kLaCand = 4;
constexpr int kLaTableWords = 4;
// slices a node pool may have: ka_search_expand writes slice t of it for the tree search (16 expansions at the most) and for
// the visit-count search (64 simulations at the most)
constexpr int kPoolMaxSlices = 64;

__host__ __device__ constexpr int la_words(int width) { return kLaCand + 3 * width; }

// the controls of model m as the kernels read them: the width (0 = off) and the prior weight
__device__ __forceinline__ int la_controls(const uint32_t* table, int m, int K, float* pw, int* skip) {
    *pw = 0.f; *skip = 0;
    if (m < 0 || m >= K) return 0;
    const uint32_t* c = table + (size_t)m * kLaTableWords;
    const int w = (int)c[0], s = (int)c[2];
    const float p = __uint_as_float(c[1]);
    if (!(w >= 0 && w <= kLaMaxWidth && p >= 0.f && p <= 3.0e38f && s >= 0)) return 0;
    *pw = p; *skip = s;
    return w;
}

// P(L) - P(W) of the value logits of row c; a non-finite logit sets *bad
__device__ __forceinline__ float la_loss_minus_win(const float* vl, size_t c, bool* bad) {
    const float l0 = vl[c * 3], l1 = vl[c * 3 + 1], l2 = vl[c * 3 + 2];
    const float mx = fmaxf(l0, fmaxf(l1, l2));
    const float e0 = expf(l0 - mx), e1 = expf(l1 - mx), e2 = expf(l2 - mx);
    *bad = !(fabsf(l0) <= 3.4e38f && fabsf(l1) <= 3.4e38f && fabsf(l2) <= 3.4e38f);
    return (e2 - e0) / (e0 + e1 + e2);
}
