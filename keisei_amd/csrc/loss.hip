// Fused KataGo-PPO minibatch loss: masked log-softmax over the 11 259 spatial actions, log-prob
// gather, clipped surrogate, entropy over legal actions, W/D/L cross-entropy (ignore_index -1,
// all-ignored guard), score MSE -- forward values AND the gradients w.r.t. the three model
// outputs in one pass, with the reference's two guards (NaN logits / zero legal actions) as
// device flags instead of host syncs.
//
// policy_loss_kernel: one workgroup per sample; the 45 KB logit row and its legal mask are
// staged once in LDS, so HBM sees one read of logits+mask and one write of dlogits.  Rows,
// masks and per-sample scalars are fetched through the minibatch index vector, i.e. the
// reference's gather (katago_ppo.py:835-841) is fused into the consumers.
//
// Reference: keisei/training/katago_ppo.py:33-57 (ppo_clip_loss, wdl_cross_entropy_loss),
// :857-924 (loss assembly), value_adapter.py:98-126; gradients follow torch autograd
// (torch.minimum ties split 1/2-1/2, clamp passes gradient on the closed interval).
//
// The masked row -- the mask read, the staged row of the softmax and the samplers, the normaliser, the draw with its uniform
// and the endings -- is csrc/policy_row.h's, shared with sampling.hip, insight.hip and lookahead.hip; the float reductions
// are common.h's ka_block_sum / ka_block_max.
#include "policy_row.h"

namespace {

constexpr int kPolThreads = 256;

struct PolicyArgs {
    const float* logits;      // (B,A)
    const uint8_t* legal;     // (S,A) bool rows, or -- legal_words > 0 -- (S,legal_words) uint32 rows, bit j of word w =
                              // action 32 w + j (the device rollout store's packing, rollout.hip); row idx[b]
    const long long* actions; // (S)
    const float* old_lp;      // (S)
    const float* adv;         // (S)
    const long long* idx;     // (B) or null (identity)
    float* dlogits;           // (B,A) or null
    float* new_lp;            // (B)
    float* rowloss;           // (B)  -min(surr1,surr2)
    float* rowent;            // (B)
    int* flags;               // [0]=NaN in logits, [1] bit 0 = zero legal actions, bit 1 = action id outside [0, A)
    const float* gscale;      // device scalar: loss scale (GradScaler) or null (=1)
    float clip_eps, w_policy, w_entropy;   // w_* already divided by B
    int A, legal_words;
};

__global__ __launch_bounds__(kPolThreads) void policy_loss_kernel(PolicyArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    uint8_t* msk = reinterpret_cast<uint8_t*>(smem + policy_row_bytes(a.A));
    __shared__ float red[kPolThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long src = a.idx ? a.idx[b] : b;
    const float* lg = a.logits + (size_t)b * a.A;
    const uint8_t* lm = a.legal + (size_t)src * a.A;
    const uint32_t* lw = reinterpret_cast<const uint32_t*>(a.legal) + (size_t)src * a.legal_words;

    float mx = -INFINITY, nlegal = 0.f;
    int nan_seen = 0;
    // four logits and mask entries are requested before the first is used (the row is one HBM round trip per pass otherwise)
    for (int j0 = tid; j0 < a.A; j0 += 4 * kPolThreads) {
        float v[4]; uint8_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * kPolThreads;
            v[u] = j < a.A ? lg[j] : 0.f;
            k[u] = j < a.A ? policy_legal(lm, lw, a.legal_words, j) : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * kPolThreads;
            if (j >= a.A) break;
            row[j] = v[u]; msk[j] = k[u];
            nan_seen |= (v[u] != v[u]);
            if (k[u]) { mx = fmaxf(mx, v[u]); nlegal += 1.f; }
        }
    }
    mx = ka_block_max<kPolThreads>(mx, red);
    nlegal = ka_block_sum<kPolThreads>(nlegal, red);
    const float nanf_ = ka_block_sum<kPolThreads>((float)nan_seen, red);
    if (tid == 0) {
        if (nanf_ > 0.f) atomicOr(&a.flags[0], 1);
        if (nlegal == 0.f) atomicOr(&a.flags[1], 1);
    }
    // The REPORTED entropy is taken from the logits relative to the maximum, log s - sum e (z - mx) / s.  As lse - sum e z / s
    // it is the difference of two numbers of the logits' magnitude and carries their ulp (1e-5 at |z| ~ 60) whatever its own
    // size.  The gradient below keeps that second form, H: there the error is multiplied by w_entropy * p, far below the
    // gradient's own rounding, and a minibatch step stays what it was to the bit.
    float s = 0.f, t = 0.f, td = 0.f;
    for (int j = tid; j < a.A; j += kPolThreads)
        if (msk[j]) {
            const float d = row[j] - mx, e = expf(d);
            s += e; td += e * d;
            {   // the product is rounded before it is added (no fused multiply-add): the sum the gradient has always used
#pragma clang fp contract(off)
                t += e * row[j];
            }
        }
    s = ka_block_sum<kPolThreads>(s, red);
    t = ka_block_sum<kPolThreads>(t, red);
    td = ka_block_sum<kPolThreads>(td, red);
    const float logs = logf(s);
    const float lse = mx + logs;
    const float H = lse - t / s;
    const float H_out = logs - td / s;
    // an action id outside [0, A) (the reference's gather would trap on the device) is flagged and read as action 0
    const long long act_raw = a.actions[src];
    const bool act_ok = act_raw >= 0 && act_raw < a.A;
    if (!act_ok && tid == 0) atomicOr(&a.flags[1], 2);
    const long long act = act_ok ? act_raw : 0;
    const float nlp = msk[act] ? row[act] - lse : -INFINITY;
    const float adv = a.adv[src];
    const float ratio = expf(nlp - a.old_lp[src]);
    const float lo = 1.f - a.clip_eps, hi = 1.f + a.clip_eps;
    const float s1 = ratio * adv, s2 = fminf(fmaxf(ratio, lo), hi) * adv;
    const bool inrange = ratio >= lo && ratio <= hi;
    float gr;                                   // d min(s1,s2) / d ratio
    if (s1 < s2) gr = adv;
    else if (s1 > s2) gr = inrange ? adv : 0.f;
    else gr = 0.5f * adv + (inrange ? 0.5f * adv : 0.f);
    if (tid == 0) { a.new_lp[b] = nlp; a.rowloss[b] = -fminf(s1, s2); a.rowent[b] = H_out; }
    if (a.dlogits) {
        // the loss scale multiplies the FINISHED gradient: a power-of-two scale then gives scale x the unscaled gradient to the
        // bit, also where w * p underflows to a subnormal (scaled weights would round those products on a finer grid)
        const float gs = a.gscale ? *a.gscale : 1.f;
        const float dnlp = -gr * ratio * a.w_policy;          // dL/d new_log_prob
        const float we = a.w_entropy;
        float* dl = a.dlogits + (size_t)b * a.A;
        for (int j = tid; j < a.A; j += kPolThreads) {
            float g = 0.f;
            if (msk[j]) {
                const float lp = row[j] - lse, p = expf(lp);
                g = -dnlp * p + we * p * (lp + H);
                if (j == act) g += dnlp;
            }
            dl[j] = g * gs;
        }
    }
}

// Rollout action selection (katago_ppo.py:566-584): probs[b] = softmax of the logits over the legal actions (0 elsewhere),
// nlegal[b] = number of legal actions.  One pass over the LDS-staged row replaces the reference's sum / masked_fill /
// softmax / renormalise / clamp / log chain of ~10 launches; sampling itself stays torch.multinomial on these rows.
// legal: bool rows (legal_words == 0) or packed rows as in ka_policy_loss.  flags[0] |= NaN in the logits.
__global__ __launch_bounds__(kPolThreads) void masked_softmax_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ legal,
                                                                     float* __restrict__ probs, int* __restrict__ nlegal_out,
                                                                     int* __restrict__ flags, int A, int legal_words) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    uint8_t* msk = reinterpret_cast<uint8_t*>(smem + policy_row_bytes(A));
    __shared__ float red[kPolThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    PolicyRowHead h = policy_stage<kPolThreads, false, false>(logits, 0, legal, legal_words, b, A, row, msk, nullptr);
    h.reduce<kPolThreads>(red);
    const float mx = h.mx;
    const float s = policy_normaliser<kPolThreads>(A, [&](int j) { return msk[j] != 0; }, [&](int j) { return expf(row[j] - mx); }, red);
    if (tid == 0) {
        if (h.nan > 0.f) atomicOr(&flags[0], 1);
        nlegal_out[b] = (int)h.nlegal;
    }
    const float inv = 1.f / s;
    float* pr = probs + (size_t)b * A;
    for (int j = tid; j < A; j += kPolThreads) pr[j] = msk[j] ? expf(row[j] - mx) * inv : 0.f;
}

// Supervised policy head (keisei/sl/trainer.py:150-152, F.cross_entropy over all A actions, mean over the batch): one
// workgroup per sample stages the logit row in LDS, rowloss[b] = logsumexp(row) - row[target[b]] and
// dlogits = w * (softmax(row) - onehot(target)), w = lambda_policy / B (times the loss scale).  flags[0] |= NaN in the logits,
// flags[1] |= a target outside [0, A).
struct PolicyCeArgs {
    const float* logits; const long long* targets; const long long* idx; float* dlogits; float* rowloss; int* flags;
    const float* gscale; float w_policy; int A;
};

// The row pass of the supervised policy head, shared by policy_ce_kernel and policy_ce_soft_kernel: the A logits at lg staged
// in LDS, their maximum, the sum of exp(z - mx) and lse = mx + log(sum); *nan_count > 0 where the row holds a NaN.
__device__ __forceinline__ float policy_ce_row_pass(const float* __restrict__ lg, int A, float* row, float* red, float* nan_count) {
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    int nan_seen = 0;
    for (int j = tid; j < A; j += kPolThreads) {
        const float v = lg[j];
        row[j] = v;
        nan_seen |= (v != v);
        mx = fmaxf(mx, v);
    }
    mx = ka_block_max<kPolThreads>(mx, red);
    *nan_count = ka_block_sum<kPolThreads>((float)nan_seen, red);
    float s = 0.f;
    for (int j = tid; j < A; j += kPolThreads) s += expf(row[j] - mx);
    s = ka_block_sum<kPolThreads>(s, red);
    return mx + logf(s);
}

__global__ __launch_bounds__(kPolThreads) void policy_ce_kernel(PolicyCeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ float red[kPolThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long src = a.idx ? a.idx[b] : b;
    float nanf_;
    const float lse = policy_ce_row_pass(a.logits + (size_t)b * a.A, a.A, row, red, &nanf_);
    const long long tgt = a.targets[src];
    const bool ok = tgt >= 0 && tgt < a.A;
    if (tid == 0) {
        if (nanf_ > 0.f) atomicOr(&a.flags[0], 1);
        if (!ok) atomicOr(&a.flags[1], 1);
        a.rowloss[b] = ok ? lse - row[tgt] : 0.f;
    }
    if (a.dlogits) {
        const float w = a.w_policy * (a.gscale ? *a.gscale : 1.f);
        float* dl = a.dlogits + (size_t)b * a.A;
        for (int j = tid; j < a.A; j += kPolThreads) {
            float g = w * expf(row[j] - lse);
            if (j == tgt) g -= w;
            dl[j] = g;
        }
    }
}

// The policy head against a distribution over at most kSoftSlots actions per row (visit counts of a search): row b has K
// slots (actions[b][k], weights[b][k]); a slot is used where its weight is > 0, and a slot of weight 0 is ignored whatever
// its action.  With W = sum of the used weights, in slot order,
//   rowloss[b]    = sum_k w_k (lse - z[a_k])                                   thread 0, in slot order
//   dlogits[b][j] = s W exp(z_j - lse) - s sum_{k: a_k = j} w_k,  s = w_policy * gscale
// The gradient is written in two steps: every element as (s W) * exp(z_j - lse), then, behind a barrier, the lowest slot of
// every distinct used action rewrites its element as fma(s W, exp(z_a - lse), -(s * sum of that action's weights in slot
// order)) -- the form policy_ce_kernel's element takes at its target, so a row whose only used slot has weight 1 gives
// ka_policy_ce's bits.  flags[1]: a used slot's action outside [0, A), a weight that is negative or not finite, or no used
// slot at all; such a row gives rowloss 0 and a zero gradient row.
constexpr int kSoftSlots = 64;

struct PolicyCeSoftArgs {
    const float* logits; const int* actions; const float* weights; int K; float* dlogits; float* rowloss; int* flags;
    const float* gscale; float w_policy; int A;
};

__global__ __launch_bounds__(kPolThreads) void policy_ce_soft_kernel(PolicyCeSoftArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ float red[kPolThreads / 64];
    __shared__ int s_act[kSoftSlots];
    __shared__ float s_w[kSoftSlots];
    __shared__ int s_state[2];                                 // a slot that is an error; a slot that is used
    __shared__ float s_total;
    const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
    float nanf_;
    const float lse = policy_ce_row_pass(a.logits + (size_t)b * a.A, a.A, row, red, &nanf_);
    if (tid < 64) {                                            // wave 0, every lane: the ballots are over the whole wave
        int act = -1;
        float w = 0.f;
        bool bad = false;
        if (tid < K) {
            act = a.actions[(size_t)b * K + tid];
            w = a.weights[(size_t)b * K + tid];
            const bool finite = fabsf(w) <= 3.4028234663852886e38f;     // false for a NaN and for an infinity
            bad = !finite || w < 0.f || (w > 0.f && (act < 0 || act >= a.A));
            if (!(w > 0.f) || bad) { w = 0.f; act = -1; }
        }
        s_act[tid] = act;
        s_w[tid] = w;
        const unsigned long long any_bad = __ballot(bad), any_used = __ballot(w > 0.f);
        if (tid == 0) { s_state[0] = any_bad != 0ull; s_state[1] = any_used != 0ull; }
    }
    __syncthreads();
    const bool valid = !s_state[0] && s_state[1];
    if (tid == 0) {
        float total = 0.f, loss = 0.f;
        if (valid)
            for (int k = 0; k < K; ++k)
                if (s_w[k] > 0.f) { total += s_w[k]; loss += s_w[k] * (lse - row[s_act[k]]); }
        s_total = total;
        if (nanf_ > 0.f) atomicOr(&a.flags[0], 1);
        if (!valid) atomicOr(&a.flags[1], 1);
        a.rowloss[b] = loss;
    }
    if (!a.dlogits) return;
    __syncthreads();
    const float s = a.w_policy * (a.gscale ? *a.gscale : 1.f);
    const float sw = s * s_total;
    float* dl = a.dlogits + (size_t)b * a.A;
    if (!valid) {
        for (int j = tid; j < a.A; j += kPolThreads) dl[j] = 0.f;
        return;
    }
    for (int j = tid; j < a.A; j += kPolThreads) dl[j] = sw * expf(row[j] - lse);
    __syncthreads();                                           // the owners below rewrite elements other threads wrote
    if (tid < K && s_w[tid] > 0.f) {
        const int act = s_act[tid];
        bool owner = true;
        float mine = 0.f;
        for (int k = 0; k < K; ++k)
            if (s_w[k] > 0.f && s_act[k] == act) {
                if (k < tid) owner = false;
                mine += s_w[k];
            }
        if (owner) dl[act] = __fmaf_rn(sw, expf(row[act] - lse), -(s * mine));
    }
}

struct ValueArgs {
    const float* vlogits;      // (B,3)
    const float* score;        // (B)
    const long long* cats;     // (S)
    const float* targets;      // (S)
    const long long* idx;      // (B) or null
    const float* rowloss;      // (B) from policy kernel
    const float* rowent;       // (B)
    float* dvlogits;           // (B,3) or null
    float* dscore;             // (B)
    float* out;                // [8]: policy, value_ce, score_mse, entropy, total, value_acc_count.. see below
    float* acc;                // [4] running sums: policy, value(combined or ce), score, entropy   (or null)
    const float* gscale;
    float lambda_policy, lambda_value, lambda_score, entropy_coeff;
    int B, combined_value_metric;
};

// single workgroup: B is a minibatch (<= a few 10^4); fixed-order reductions
__global__ __launch_bounds__(1024) void value_loss_kernel(ValueArgs a) {
    __shared__ double red[8][16];
    const int tid = threadIdx.x;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // nvalid, ce, mse, pl, ent, correct, pred0, pred1
    for (int b = tid; b < a.B; b += 1024) {
        const long long src = a.idx ? a.idx[b] : b;
        const float l0 = a.vlogits[b * 3], l1 = a.vlogits[b * 3 + 1], l2 = a.vlogits[b * 3 + 2];
        const long long cat = a.cats[src];
        const float m = fmaxf(l0, fmaxf(l1, l2));
        const float lse = m + logf(expf(l0 - m) + expf(l1 - m) + expf(l2 - m));
        if (cat >= 0) {
            acc[0] += 1.0;
            acc[1] += (double)(lse - (cat == 0 ? l0 : (cat == 1 ? l1 : l2)));
            const int pred = (l0 >= l1 && l0 >= l2) ? 0 : (l1 >= l2 ? 1 : 2);
            acc[5] += pred == cat; acc[6] += pred == 0; acc[7] += pred == 1;
        }
        const float d = a.score[b] - a.targets[src];
        acc[2] += (double)(d * d);
        acc[3] += (double)a.rowloss[b];
        acc[4] += (double)a.rowent[b];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        acc[k] = wave_sum_d(acc[k]);
        if ((tid & 63) == 0) red[k][tid >> 6] = acc[k];
    }
    __syncthreads();
    double tot[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { tot[k] = 0; for (int w = 0; w < 16; ++w) tot[k] += red[k][w]; }
    const double nvalid = tot[0];
    const float ce = nvalid > 0 ? (float)(tot[1] / nvalid) : 0.f;
    const float mse = (float)(tot[2] / a.B), pl = (float)(tot[3] / a.B), ent = (float)(tot[4] / a.B);
    if (tid == 0) {
        const float vs = a.lambda_value * ce + a.lambda_score * mse;
        a.out[0] = pl; a.out[1] = ce; a.out[2] = mse; a.out[3] = ent;
        a.out[4] = a.lambda_policy * pl + vs - a.entropy_coeff * ent;
        a.out[5] = (float)nvalid;
        a.out[6] = nvalid > 0 ? (float)(tot[5] / nvalid) : 0.f;            // value_accuracy
        a.out[7] = nvalid > 0 ? (float)(tot[6] / nvalid) : 0.f;            // frac_predicted_win
        a.out[8] = nvalid > 0 ? (float)(tot[7] / nvalid) : 0.f;            // frac_predicted_draw
        if (a.acc) {
            a.acc[0] += pl;
            a.acc[1] += a.combined_value_metric ? vs : ce;
            a.acc[2] += a.combined_value_metric ? 0.f : mse;
            a.acc[3] += ent;
        }
    }
    if (a.dvlogits) {
        const float gs = a.gscale ? *a.gscale : 1.f;
        const float wv = nvalid > 0 ? (float)(a.lambda_value / nvalid) * gs : 0.f;
        const float ws = 2.f * a.lambda_score / a.B * gs;
        for (int b = tid; b < a.B; b += 1024) {
            const long long src = a.idx ? a.idx[b] : b;
            const long long cat = a.cats[src];
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (cat >= 0) {
                const float l0 = a.vlogits[b * 3], l1 = a.vlogits[b * 3 + 1], l2 = a.vlogits[b * 3 + 2];
                const float m = fmaxf(l0, fmaxf(l1, l2));
                const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m), inv = 1.f / (e0 + e1 + e2);
                g0 = (e0 * inv - (cat == 0)) * wv; g1 = (e1 * inv - (cat == 1)) * wv; g2 = (e2 * inv - (cat == 2)) * wv;
            }
            a.dvlogits[b * 3] = g0; a.dvlogits[b * 3 + 1] = g1; a.dvlogits[b * 3 + 2] = g2;
            a.dscore[b] = ws * (a.score[b] - a.targets[src]);
        }
    }
}

// Held-out evaluation of the supervised heads (SLTrainer.evaluate): no gradient, sums over positions instead of batch means.
// sl_eval_rows_kernel is policy_ce_kernel's row pass -- one workgroup per sample, the logit row staged in LDS, rowloss[b] =
// logsumexp(row) - row[t] -- and, from the same staged row, the target's place in a stable descending sort:
//   rank[b] = #{j : z_j > z_t} + #{j < t : z_j == z_t}
// (an integer count, whatever the order of the threads).  A target outside [0, A) gives rowloss 0, rank A and flags[1].
// sl_eval_reduce_kernel is one workgroup, as value_loss_kernel: per row the W/D/L cross-entropy and the argmax by its rule,
// the squared score error, top-1 = rank 0, top-k = rank < k; per-thread sums in double over b, b + 1024, ..., a wave
// reduction, the 16 waves added in order by thread 0, and thread 0 alone adds the batch into the accumulator -- launches
// are ordered by the stream, so two runs give the same bits and nothing needs a float atomic.
struct SlEvalArgs {
    const float* logits; const float* vlogits; const float* score;
    const long long* policy_t; const long long* value_t; const float* score_t;
    float* rowloss; int* rank; long long* acc_i; double* acc_f; int* flags; int B, A, k;
};

__global__ __launch_bounds__(kPolThreads) void sl_eval_rows_kernel(SlEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ float red[kPolThreads / 64];
    __shared__ int redi[kPolThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* lg = a.logits + (size_t)b * a.A;
    float mx = -INFINITY;
    int nan_seen = 0;
    for (int j = tid; j < a.A; j += kPolThreads) {
        const float v = lg[j];
        row[j] = v;
        nan_seen |= (v != v);
        mx = fmaxf(mx, v);
    }
    mx = ka_block_max<kPolThreads>(mx, red);
    const float nanf_ = ka_block_sum<kPolThreads>((float)nan_seen, red);
    float s = 0.f;
    for (int j = tid; j < a.A; j += kPolThreads) s += expf(row[j] - mx);
    s = ka_block_sum<kPolThreads>(s, red);
    const float lse = mx + logf(s);
    const long long tgt = a.policy_t[b];
    const bool ok = tgt >= 0 && tgt < a.A;
    const float zt = ok ? row[tgt] : 0.f;
    int above = 0;
    if (ok)
        for (int j = tid; j < a.A; j += kPolThreads) {
            const float v = row[j];
            above += (v > zt) || (v == zt && j < tgt);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
    if ((tid & 63) == 0) redi[tid >> 6] = above;
    __syncthreads();
    if (tid == 0) {
        int rank = 0;
        for (int w = 0; w < kPolThreads / 64; ++w) rank += redi[w];
        if (nanf_ > 0.f) atomicOr(&a.flags[0], 1);
        if (!ok) atomicOr(&a.flags[1], 1);
        a.rowloss[b] = ok ? lse - zt : 0.f;
        a.rank[b] = ok ? rank : a.A;
    }
}

__global__ __launch_bounds__(1024) void sl_eval_reduce_kernel(SlEvalArgs a) {
    __shared__ double redd[3][16];
    __shared__ int redi[3][16];
    const int tid = threadIdx.x;
    double sum[3] = {0, 0, 0};                  // policy CE, value CE, squared score error
    int cnt[3] = {0, 0, 0};                     // top-1, top-k, value prediction right
    int nan_seen = 0, bad = 0;
    for (int b = tid; b < a.B; b += 1024) {
        const float l0 = a.vlogits[b * 3], l1 = a.vlogits[b * 3 + 1], l2 = a.vlogits[b * 3 + 2], sc = a.score[b];
        nan_seen |= (l0 != l0) | (l1 != l1) | (l2 != l2) | (sc != sc);
        const long long cat = a.value_t[b];
        if (cat >= 0 && cat <= 2) {
            const float m = fmaxf(l0, fmaxf(l1, l2));
            const float lse = m + logf(expf(l0 - m) + expf(l1 - m) + expf(l2 - m));
            sum[1] += (double)(lse - (cat == 0 ? l0 : (cat == 1 ? l1 : l2)));
            const int pred = (l0 >= l1 && l0 >= l2) ? 0 : (l1 >= l2 ? 1 : 2);
            cnt[2] += pred == cat;
        } else {
            bad = 1;
        }
        const float d = sc - a.score_t[b];
        sum[2] += (double)(d * d);
        sum[0] += (double)a.rowloss[b];
        const int rank = a.rank[b];
        cnt[0] += rank == 0;
        cnt[1] += rank < a.k;
    }
    if (nan_seen) atomicOr(&a.flags[0], 1);
    if (bad) atomicOr(&a.flags[1], 1);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        sum[q] = wave_sum_d(sum[q]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[q] += __shfl_xor(cnt[q], o);
        if ((tid & 63) == 0) { redd[q][tid >> 6] = sum[q]; redi[q][tid >> 6] = cnt[q]; }
    }
    __syncthreads();
    if (tid == 0) {
        a.acc_i[0] += a.B;
        for (int q = 0; q < 3; ++q) {
            double t = 0;
            long long c = 0;
            for (int w = 0; w < 16; ++w) { t += redd[q][w]; c += redi[q][w]; }
            a.acc_i[1 + q] += c;
            a.acc_f[q] += t;
        }
    }
}

// rollout side: scalar value P(W)-P(L) (+ optional blend with clamp(score,-1,1))
__global__ void scalar_value_kernel(const float* __restrict__ vl, const float* __restrict__ score, float alpha,
                                    float* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[b] = ka_blended_value(vl + b * 3, score ? score + b : nullptr, alpha);
}

// Rollout side, one launch per select_actions call (katago_ppo.py:567-612: masked_fill(-inf) -> softmax -> Categorical.sample()
// -> log_prob, zero-legal guard, scalar value): one workgroup per environment stages the logit row in LDS, draws ONE action
// by inverse-CDF over the legal actions (contiguous chunk per thread, block prefix sums, the first chunk whose running
// total passes u * total is walked) and returns log p(action) as the masked-softmax path does; the value head's
// P(W) - P(L) (+ blend) rides along.  u comes from a 64-bit mix of (seed, environment): the caller draws `seed` from the
// host generator, so torch.manual_seed() still fixes the rollout.  flags[0] |= NaN logits, flags[1] |= a row without a
// legal action (its action is 0, the caller raises as the reference does).
//
// The play form (Play = true, ka_policy_sample_play) reads the seed from device memory, so a captured graph draws fresh
// randomness on every replay, and takes each row's model index: a row whose model_of[b] lies outside [0, K) gets its first
// legal action and log-prob 0 (the reference's legal_masks.argmax(-1) for idle partitions, concurrent_matches.py:388-404).
// Seated rows run the same arithmetic as the plain form: the same seed value gives the same actions and log-probs.
struct SampleArgs {
    const void* logits; int logits_bf16; const uint8_t* legal; int legal_words; unsigned long long seed;
    const float* vlogits; const float* score; float alpha;
    long long* actions; float* logp; float* values; int* nlegal; int* flags; int A;
    const long long* seed_dev; const int* model_of; int K;      // play form only
};

template <bool Play>
__global__ __launch_bounds__(kPolThreads) void policy_sample_kernel(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* row = reinterpret_cast<float*>(smem);
    uint8_t* msk = reinterpret_cast<uint8_t*>(smem + policy_row_bytes(a.A));
    __shared__ float red[kPolThreads / 64];
    __shared__ PolicyDrawLds<kPolThreads> draw;
    const int b = blockIdx.x, tid = threadIdx.x, A = a.A;
    PolicyRowHead h = policy_stage<kPolThreads, Play, false>(a.logits, a.logits_bf16, a.legal, a.legal_words, b, A, row, msk, nullptr);
    draw.reset(A);
    h.reduce<kPolThreads>(red);
    if constexpr (Play) {
        const int m = a.model_of[b];
        if (m < 0 || m >= a.K) {                               // unseated row (uniform over the workgroup)
            policy_end_unseated(h, A, draw, a.flags, &a.nlegal[b], &a.actions[b], &a.logp[b]);
            return;
        }
    }
    const float mx = h.mx;
    const auto legal = [&](int j) { return msk[j] != 0; };
    const auto weight = [&](int j) { return expf(row[j] - mx); };
    const float s = policy_normaliser<kPolThreads>(A, legal, weight, red);   // the normaliser of the masked-softmax path (same order)
    const unsigned long long seed = Play ? (unsigned long long)*a.seed_dev : a.seed;
    policy_draw(A, b, seed, s, legal, weight, draw, &a.actions[b], &a.logp[b]);
    if (tid == 0) {
        policy_report(h, a.flags, &a.nlegal[b], &a.actions[b], &a.logp[b]);
        if (a.values)                                          // katago_ppo.py:536-541 / value_adapter.py:56-65
            a.values[b] = ka_blended_value(a.vlogits + b * 3, a.score ? a.score + b : nullptr, a.alpha);
    }
}

}  // namespace

extern "C" int ka_policy_loss(const float* logits, const void* legal, const long long* actions, const float* old_lp,
                              const float* adv, const long long* idx, float* dlogits, float* new_lp, float* rowloss,
                              float* rowent, int* flags, const float* gscale, float clip_eps, float w_policy,
                              float w_entropy, int B, int A, int legal_words, void* stream) {
    KA_REQUIRE(logits && legal && actions && old_lp && adv && new_lp && rowloss && rowent && flags && B > 0 && A > 0,
               "policy_loss: null tensor");
    KA_REQUIRE_MASK_ROW("policy_loss", A, legal_words);
    PolicyArgs a{logits, static_cast<const uint8_t*>(legal), actions, old_lp, adv, idx, dlogits, new_lp, rowloss,
                 rowent, flags, gscale, clip_eps, w_policy, w_entropy, A, legal_words};
    const size_t lds = policy_row_bytes(A) + policy_mask_bytes(A);
    KA_REQUIRE_ROW_LDS("policy_loss", lds, A);
    hipLaunchKernelGGL(policy_loss_kernel, dim3(B), dim3(kPolThreads), lds, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_loss");
}

extern "C" int ka_masked_softmax(const float* logits, const void* legal, float* probs, int* nlegal, int* flags, int B, int A,
                                 int legal_words, void* stream) {
    KA_REQUIRE(logits && legal && probs && nlegal && flags && B > 0 && A > 0, "masked_softmax: null tensor");
    KA_REQUIRE_MASK_ROW("masked_softmax", A, legal_words);
    const size_t lds = policy_row_bytes(A) + policy_mask_bytes(A);
    KA_REQUIRE_ROW_LDS("masked_softmax", lds, A);
    hipLaunchKernelGGL(masked_softmax_kernel, dim3(B), dim3(kPolThreads), lds, static_cast<hipStream_t>(stream), logits,
                       static_cast<const uint8_t*>(legal), probs, nlegal, flags, A, legal_words);
    return ka_check_launch("masked_softmax");
}

extern "C" int ka_policy_sample(const void* logits, int logits_bf16, const void* legal, int legal_words, long long seed,
                                const float* vlogits, const float* score, float alpha, long long* actions, float* logp,
                                float* values, int* nlegal, int* flags, int B, int A, void* stream) {
    KA_REQUIRE(logits && legal && actions && logp && nlegal && flags && B > 0 && A > 0, "policy_sample: null tensor");
    KA_REQUIRE_MASK_ROW("policy_sample", A, legal_words);
    KA_REQUIRE((values == nullptr) || vlogits, "policy_sample: values need the value logits");
    const size_t lds = policy_row_bytes(A) + policy_mask_bytes(A);
    KA_REQUIRE_ROW_LDS("policy_sample", lds, A);
    SampleArgs a{logits, logits_bf16, static_cast<const uint8_t*>(legal), legal_words, (unsigned long long)seed, vlogits, score, alpha,
                 actions, logp, values, nlegal, flags, A, nullptr, nullptr, 0};
    hipLaunchKernelGGL(policy_sample_kernel<false>, dim3(B), dim3(kPolThreads), lds, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_sample");
}

extern "C" int ka_policy_sample_play(const void* logits, int logits_bf16, const void* legal, int legal_words,
                                     const long long* seed_dev, const int* model_of, int K, long long* actions, float* logp,
                                     int* nlegal, int* flags, int B, int A, void* stream) {
    KA_REQUIRE(logits && legal && seed_dev && model_of && actions && logp && nlegal && flags && B > 0 && A > 0,
               "policy_sample_play: null tensor");
    KA_REQUIRE_MASK_ROW("policy_sample_play", A, legal_words);
    const size_t lds = policy_row_bytes(A) + policy_mask_bytes(A);
    KA_REQUIRE_ROW_LDS("policy_sample_play", lds, A);
    SampleArgs a{logits, logits_bf16, static_cast<const uint8_t*>(legal), legal_words, 0ull, nullptr, nullptr, 0.f,
                 actions, logp, nullptr, nlegal, flags, A, seed_dev, model_of, K};
    hipLaunchKernelGGL(policy_sample_kernel<true>, dim3(B), dim3(kPolThreads), lds, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_sample_play");
}

extern "C" int ka_policy_ce(const float* logits, const long long* targets, const long long* idx, float* dlogits,
                            float* rowloss, int* flags, const float* gscale, float w_policy, int B, int A, void* stream) {
    KA_REQUIRE(logits && targets && rowloss && flags && B > 0 && A > 0, "policy_ce: null tensor");
    PolicyCeArgs a{logits, targets, idx, dlogits, rowloss, flags, gscale, w_policy, A};
    const size_t lds = policy_row_bytes(A);
    KA_REQUIRE_ROW_LDS("policy_ce", lds, A);
    hipLaunchKernelGGL(policy_ce_kernel, dim3(B), dim3(kPolThreads), lds, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_ce");
}

extern "C" int ka_policy_ce_soft(const float* logits, const int* actions, const float* weights, int K, float* dlogits,
                                 float* rowloss, int* flags, const float* gscale, float w_policy, int B, int A, void* stream) {
    KA_REQUIRE(logits && actions && weights && rowloss && flags && B > 0 && A > 0, "policy_ce_soft: null tensor");
    KA_REQUIRE(K >= 1 && K <= kSoftSlots, "policy_ce_soft: K %d (1..%d)", K, kSoftSlots);
    PolicyCeSoftArgs a{logits, actions, weights, K, dlogits, rowloss, flags, gscale, w_policy, A};
    const size_t lds = policy_row_bytes(A);
    KA_REQUIRE(lds <= 63 * 1024, "policy_ce_soft: action space %d too large for the LDS row", A);
    hipLaunchKernelGGL(policy_ce_soft_kernel, dim3(B), dim3(kPolThreads), lds, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("policy_ce_soft");
}

// out[9]: policy_loss, value_ce, score_mse, entropy, total, n_valid, value_accuracy, frac_win, frac_draw
extern "C" int ka_value_loss(const float* vlogits, const float* score, const long long* cats, const float* targets,
                             const long long* idx, const float* rowloss, const float* rowent, float* dvlogits,
                             float* dscore, float* out, float* acc, const float* gscale, float lambda_policy,
                             float lambda_value, float lambda_score, float entropy_coeff, int combined_value_metric,
                             int B, void* stream) {
    KA_REQUIRE(vlogits && score && cats && targets && rowloss && rowent && out && B > 0, "value_loss: null tensor");
    KA_REQUIRE((dvlogits == nullptr) == (dscore == nullptr), "value_loss: dvlogits/dscore must come together");
    ValueArgs a{vlogits, score, cats, targets, idx, rowloss, rowent, dvlogits, dscore, out, acc, gscale,
                lambda_policy, lambda_value, lambda_score, entropy_coeff, B, combined_value_metric};
    hipLaunchKernelGGL(value_loss_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("value_loss");
}

extern "C" int ka_sl_eval(const float* logits, const float* vlogits, const float* score, const long long* policy_t,
                          const long long* value_t, const float* score_t, int B, int A, int k, float* rowloss, int* rank,
                          void* acc, int* flags, void* stream) {
    KA_REQUIRE(logits && vlogits && score && policy_t && value_t && score_t && rowloss && rank && acc && flags,
               "sl_eval: null tensor");
    KA_REQUIRE(B > 0 && A > 0, "sl_eval: B %d, A %d", B, A);
    KA_REQUIRE(k >= 1 && k <= A, "sl_eval: k %d outside [1, %d]", k, A);
    KA_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7) == 0, "sl_eval: the accumulator must be 8-byte aligned");
    const size_t lds = policy_row_bytes(A);
    KA_REQUIRE_ROW_LDS("sl_eval", lds, A);
    SlEvalArgs a{logits, vlogits, score, policy_t, value_t, score_t, rowloss, rank, static_cast<long long*>(acc),
                 reinterpret_cast<double*>(static_cast<char*>(acc) + 32), flags, B, A, k};
    hipLaunchKernelGGL(sl_eval_rows_kernel, dim3(B), dim3(kPolThreads), lds, static_cast<hipStream_t>(stream), a);
    hipLaunchKernelGGL(sl_eval_reduce_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("sl_eval");
}

extern "C" int ka_scalar_value(const float* vlogits, const float* score, float alpha, float* out, int B, void* stream) {
    KA_REQUIRE(vlogits && out && B > 0, "scalar_value: null tensor");
    hipLaunchKernelGGL(scalar_value_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       vlogits, score, alpha, out, B);
    return ka_check_launch("scalar_value");
}
