// Policy insight: what the reference's showcase shows next to a board (showcase/runner.py:151-173, showcase/heatmap.py:40-49,
// showcase/inference.py:95) -- the softmax over the legal moves at a sampling temperature, the top candidates, the heatmap of
// the chosen move's family and the win probability -- computed where the full logit row exists: on the device, in the ply,
// between the sampler and the env step.  The row lives in a workspace the next forward overwrites; copying it out would be
// 45 KB per env per ply.  Added to it: the entropy of the distribution, the rank of the chosen move and the number of legal moves.
//
// One workgroup per row.  A position has tens of legal moves out of 11 259 actions, so every pass walks the set bits of the
// mask row, not the actions: thread t owns mask words t and t + 256, reads the logits behind their set bits from memory once
// and parks them in an LDS row at the action's index (only legal positions of that row are ever written or read).  Then one
// pass for the normaliser, the entropy sum and the rank, top_k rounds of a block arg-max (each round takes the best action
// that comes after the previous winner in the order "logit descending, action ascending", so nothing is sorted and nothing
// in the row is changed), the heat row, and one record of 8 + 2 top_k words:
//   0 flags (bit 0 valid, bit 1 mover's colour, bit 2 the chosen action is legal)   1 chosen action (int32, clamped)
//   2 n_legal   3 chosen_rank (-1 where the chosen action is not legal)   4 chosen_probability   5 entropy (nats)
//   6 win_probability   7 reserved (0)   8.. top actions (int32, -1 = unused)   8 + top_k.. their probabilities (fp32)
// A row whose model_of lies outside [0, K) or that has no legal action is written as all zeros (record and heat).
// Ranks and the candidate order compare raw logits, so they do not depend on rounding; a legal logit that is -inf or NaN is
// never a candidate.  Kernel nodes only, caller-owned buffers, no workgroup waits for another.
//
// The walk over the set bits, the staged row, the candidate order and the round are csrc/policy_row.h's: the sampling
// controls' cut and the lookahead's fork run the same bodies, so their candidates are these.
#include "ply_rows.h"
#include "policy_row.h"

namespace {

constexpr int kInThreads = 256, kInWaves = kInThreads / 64;
constexpr int kInSlots = kPlySlots, kInA = kPlyA, kInWords = kPlyWords;           // csrc/ply_rows.h
constexpr int kInHeat = 132, kInMaxTop = 8;
constexpr int kInFlags = 0, kInAction = 1, kInNLegal = 2, kInRank = 3, kInProb = 4, kInEntropy = 5, kInWin = 6, kInTop = 8;

__host__ __device__ constexpr int in_words(int top_k) { return kInTop + 2 * top_k; }

struct InsightArgs {
    const void* logits; int logits_bf16; const uint32_t* legal; int legal_words; const long long* actions;
    const float* vlogits; const uint8_t* players; const int* model_of; int K; float inv_t; int top_k;
    uint32_t* last; float* heat; uint32_t* hist; int row_len; const int* count; int* flags;
};

__global__ __launch_bounds__(kInThreads) void policy_insight_kernel(InsightArgs a) {
    __shared__ float row[kInA];
    __shared__ uint32_t msk[kInWords];
    __shared__ float red[kInWaves];
    __shared__ int red_i[kInWaves];
    __shared__ uint32_t rec[in_words(kInMaxTop)];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W = in_words(a.top_k);
    uint32_t* last = a.last + (size_t)b * W;
    float* heat = a.heat + (size_t)b * kInHeat;
    uint32_t* slot = nullptr;                                  // the history entry of this move, if there is room for it
    if (a.hist) {
        const int c = a.count[b];
        if (c >= 0 && c < a.row_len) slot = a.hist + ((size_t)b * a.row_len + c) * W;
    }
    const uint32_t* lw = a.legal + (size_t)b * a.legal_words;
    const int m = a.model_of ? a.model_of[b] : 0;
    const bool seated = !a.model_of || (m >= 0 && m < a.K);    // (uniform over the workgroup)
    PolicyRowHead h{-INFINITY, 0.f, 0.f, INT_MAX};
    if (seated) {
        for (int w = tid; w < kInWords; w += kInThreads) msk[w] = mask_word(lw, w);
        h = policy_stage_legal<kInThreads>(a.logits, a.logits_bf16, (size_t)b * kInA, msk, kInWords, row);
        h.nlegal = ka_block_sum<kInThreads>(h.nlegal, red);    // (at most 11259: exact in fp32; row and msk are visible behind it)
    }
    const float nl = h.nlegal;
    if (!seated || nl == 0.f) {                                // an invalid row: all zeros
        if (tid < W) { last[tid] = 0u; if (slot) slot[tid] = 0u; }
        if (tid < kInHeat) heat[tid] = 0.f;
        return;
    }
    const float mx = ka_block_max<kInThreads>(h.mx, red);
    const float nan_any = ka_block_sum<kInThreads>(h.nan, red);
    const long long act64 = a.actions[b];
    const bool in_range = act64 >= 0 && act64 < kInA;
    const int act = in_range ? (int)act64 : (act64 < 0 ? -1 : kInA);
    const bool legal_act = in_range && ((msk[act >> 5] >> (act & 31)) & 1u);
    const float la = legal_act ? row[act] : 0.f;
    // the normaliser, the entropy sum and the rank in one pass: p = e / S, ln p = z - ln S, H = ln S - sum(e z) / S
    float s = 0.f, t = 0.f, above = 0.f;
    policy_for_legal<kInThreads>(msk, kInWords, [&](int j) {
        const float v = row[j];
        if (legal_act && v > la) above += 1.f;
        const float z = (v - mx) * a.inv_t, e = expf(z);       // (a legal logit of -inf: e = 0)
        s += e;
        if (e > 0.f) t += e * z;
    });
    s = ka_block_sum<kInThreads>(s, red);
    t = ka_block_sum<kInThreads>(t, red);
    above = ka_block_sum<kInThreads>(above, red);
    if (tid == 0) {
        if (nan_any > 0.f) atomicOr(&a.flags[0], 1);
        float win = 0.f;
        if (a.vlogits) {                                       // softmax(value_logits)[0] (showcase/inference.py:95)
            const float* vl = a.vlogits + (size_t)b * 3;
            const float vm = fmaxf(vl[0], fmaxf(vl[1], vl[2]));
            const float e0 = expf(vl[0] - vm), e1 = expf(vl[1] - vm), e2 = expf(vl[2] - vm);
            win = e0 / (e0 + e1 + e2);
        }
        const uint32_t colour = a.players ? (uint32_t)(a.players[b] & 1) : 0u;
        rec[kInFlags] = 1u | (colour << 1) | ((uint32_t)legal_act << 2);
        rec[kInAction] = (uint32_t)act;
        rec[kInNLegal] = (uint32_t)(int)nl;
        rec[kInRank] = (uint32_t)(legal_act ? (int)above : -1);
        rec[kInProb] = __float_as_uint(legal_act ? expf((la - mx) * a.inv_t) / s : 0.f);
        rec[kInEntropy] = __float_as_uint(logf(s) - t / s);
        rec[kInWin] = __float_as_uint(win);
        rec[7] = 0u;
    }
    // top candidates: round r takes the first action behind round r - 1's winner in the candidate order
    float prev_v = INFINITY;
    int prev_i = -1;
    for (int r = 0; r < a.top_k; ++r) {                        // (prev_i is uniform over the workgroup, so is every branch on it)
        float bv = -INFINITY;
        int bi = INT_MAX;
        if (r == 0 || prev_i != INT_MAX) bi = policy_next<kInThreads, false>(row, msk, kInWords, prev_v, prev_i, red, red_i, &bv);
        if (tid == 0) {
            rec[kInTop + r] = (uint32_t)(bi == INT_MAX ? -1 : bi);
            rec[kInTop + a.top_k + r] = __float_as_uint(bi == INT_MAX ? 0.f : expf((bv - mx) * a.inv_t) / s);
        }
        prev_v = bv; prev_i = bi;
    }
    // the heat row: the chosen move's family (showcase/heatmap.py:40-49: the same from-square, or the same dropped piece)
    if (tid < kInHeat) {
        float h = 0.f;
        if (legal_act) {
            const int from = act / kInSlots, sl = act % kInSlots;
            const int j = sl < kInHeat ? from * kInSlots + tid : (tid < 81 ? tid * kInSlots + sl : -1);
            if (j >= 0 && ((msk[j >> 5] >> (j & 31)) & 1u)) h = expf((row[j] - mx) * a.inv_t) / s;
        }
        heat[tid] = h;
    }
    __syncthreads();
    if (tid < W) { const uint32_t w = rec[tid]; last[tid] = w; if (slot) slot[tid] = w; }
}

}  // namespace

extern "C" int ka_policy_insight_words(int which, int top_k) {
    if (top_k < 1 || top_k > kInMaxTop) return -1;
    return which == 0 ? in_words(top_k) : which == 1 ? kInFlags : which == 2 ? kInAction : which == 3 ? kInNLegal
         : which == 4 ? kInRank : which == 5 ? kInProb : which == 6 ? kInEntropy : which == 7 ? kInWin : which == 8 ? kInTop
         : which == 9 ? kInTop + top_k : which == 10 ? kInHeat : -1;
}

extern "C" int ka_policy_insight(const void* logits, int logits_bf16, const void* legal, int legal_words, const long long* actions,
                                 const float* vlogits, const void* players, const int* model_of, int K, float temperature,
                                 int top_k, void* last, float* heat, void* hist, int row_len, const int* count, int* flags,
                                 int B, int A, void* stream) {
    KA_REQUIRE(logits && legal && actions && last && heat && flags && B > 0, "policy_insight: null tensor");
    KA_REQUIRE(A == kInA, "policy_insight: the spatial action space only (A = %d), got %d", kInA, A);
    KA_REQUIRE(legal_words == (A + 31) / 32, "policy_insight: packed mask rows of %d words", (A + 31) / 32);
    KA_REQUIRE(top_k >= 1 && top_k <= kInMaxTop, "policy_insight: top_k must lie in [1, %d], got %d", kInMaxTop, top_k);
    KA_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, "policy_insight: temperature must be positive and finite");
    KA_REQUIRE(!hist || (count && row_len > 0), "policy_insight: a history needs its counts and row_len > 0 (got %d)", row_len);
    KA_REQUIRE((uintptr_t)logits % (logits_bf16 ? 2 : 4) == 0 && (uintptr_t)legal % 4 == 0 && (uintptr_t)actions % 8 == 0 &&
               (uintptr_t)vlogits % 4 == 0 && (uintptr_t)model_of % 4 == 0 && (uintptr_t)last % 4 == 0 &&
               (uintptr_t)heat % 4 == 0 && (uintptr_t)hist % 4 == 0 && (uintptr_t)count % 4 == 0 && (uintptr_t)flags % 4 == 0,
               "policy_insight: actions are 8-byte aligned, every other tensor to its element size");
    InsightArgs a{logits, logits_bf16, static_cast<const uint32_t*>(legal), legal_words, actions, vlogits,
                  static_cast<const uint8_t*>(players), model_of, K, 1.0f / temperature, top_k, static_cast<uint32_t*>(last), heat,
                  static_cast<uint32_t*>(hist), row_len, count, flags};
    hipLaunchKernelGGL(policy_insight_kernel, dim3(B), dim3(kInThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_insight");
}
