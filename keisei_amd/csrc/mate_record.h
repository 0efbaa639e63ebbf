// The record ka_mate_fork and ka_mate_choose write per env (csrc/mate.hip states its meaning), 4 + cap int32 words.  The
// mate in three (csrc/mate3.hip) reads the root's and the third ply's records through the same names.
#pragma once
#include "common.h"

constexpr int kMtFlags = 0, kMtNChecks = 1, kMtSlot = 2, kMtAction = 3, kMtList = 4;
constexpr uint32_t kMtActive = 1u, kMtMate = 2u, kMtChanged = 4u, kMtTruncated = 8u;      // bits of the flags word

__host__ __device__ constexpr int mt_words(int cap) { return kMtList + cap; }
