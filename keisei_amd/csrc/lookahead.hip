// One-ply value lookahead in the device ply.  The reference never searches: every move of its matches is one draw from the raw
// policy.  Here a game's complete state is a few rows of device memory (a 128-byte state row plus `ply` words of key / check
// history) and the grouped forward evaluates thousands of boards of mixed models in three launches, so a one-ply search is
// "copy rows, step them with the env kernel as it is, evaluate them with the forward as it is, arg-max":
//
//   ka_lookahead_fork       the first `width` legal actions of every active env in the candidate order of the insight and the
//                           sampling controls, their priors, and one child row per candidate: state, history, mask, action
//   ka_shogi_env_step       (csrc/shogi_env.hip, unchanged) over the N * width child rows
//   grouped forward         (csrc/tower.hip, unchanged) over the child observations
//   ka_lookahead_choose     q of every child (its reward when the game ended there, else P(L) - P(W) of the child's value
//                           head: the child is seen by its side to move), u = q + prior_weight * prior, the arg-max replaces
//                           the sampler's action
//
// Row m of the controls table (device memory, read by every launch: a new table applies from the next ply of a captured
// graph) belongs to model m:   word 0 int32 width   1 fp32 prior_weight   2 int32 skip_plies   3 int32 reply_width
// A row with width outside [0, 8], a negative or non-finite weight or a negative skip_plies reads as "off"; a width above
// the launch's width is cut to it.  An env is active when its model lies in [0, K), the row's width is positive, its game
// ply (the ply word of its state row, csrc/shogi_rules.h) is at least skip_plies and it has a candidate.
//
// Record of an env, 4 + 3 width 32-bit words:
//   0 flags (bit 0 active, bit 1 the choice differs from the sampler's action, bit 2 the chosen move won the game)
//   1 chosen slot   2 n_cand   3 chosen action (the sampler's for an inactive env)
//   4.. candidate actions (int32, -1 = unused)   4 + width.. priors (fp32)   4 + 2 width.. q (fp32)
//
// The fork is one workgroup per env and walks the set bits of the packed mask row, never the action space; the copies are
// what it is for: the ply's one fork copy (csrc/ply_rows.h), shared with the mate searches.  Unused and inactive child
// slots get the state, the mask and the env's own sampled action (legal whenever the main step's is: one refused action
// makes the env step hold every row of its launch) and model -1; their history is not copied -- the env kernel only counts
// repetitions in it, and nothing reads such a child's outcome.  The parent's rows are only read.  Kernel nodes only,
// caller-owned buffers, no workgroup waits for another.
//
// Reply search (word 3 of the row, reply_width 0..8; 0 = one ply, outside the range reads as 0; ka_lookahead_fork and
// ka_lookahead_choose ignore it).  A child after the env step is again a complete env row, and the children's forward wrote
// their policy logits anyway, so a second ply is three more stages and another choice:
//
//   ka_lookahead_fork_replies     the fork kernel with the child as "env": the first reply_width legal actions of every live
//                                 child by the child's own logits, a reply record per child, the grandchild rows
//   ka_shogi_env_step, forward    unchanged, over the N * width * reply_width grandchild rows
//   ka_lookahead_choose_replies   v of every grandchild for the root mover (0 - reward where the game ended there, else
//                                 P(W) - P(L): it is seen by the root mover again), q = the first minimum over the replies
//                                 (a done child keeps its reward, a live child without replies its one-ply q), the choice as
//                                 above; flag bit 3 and stats word 3: the choice differs from the one-ply choice
//
// A reply record has the env record's layout with reply_width in the place of width: slot and action are the first worst
// reply for the mover, the q words the grandchildren's values.  A done child's row is a restarted game and gets no replies.
//
// Tree search (a table whose word 3 is `expansions`, 1..16; the block above search_advance_kernel and include/keisei_amd.h
// state it).  All forked rows of a ply lie in one pool, `width` rows per env and expansion, and every expansion after the
// env's own fork spends its rows on the leaf of the current principal variation:
//
//   ka_search_expand      the fork kernel with a row of the pool as "env", named per env by parent_row / active
//   ka_search_advance     one thread per env: leaf q, the backup by max and negation, the next leaf, at the end the choice
//
// The fork's candidates -- the walk over the set bits, the staged row, the candidate order and the round -- are
// csrc/policy_row.h's, the bodies the insight and the sampling controls run: that is why the orders are one order.
#include "lookahead_record.h"
#include "policy_row.h"

namespace {

constexpr int kLaThreads = 256, kLaWaves = kLaThreads / 64;
constexpr int kLaStatsWords = 4;

struct ForkArgs {
    const void* logits; int logits_bf16; const uint32_t* legal; const long long* actions; const int* model_of; int K;
    const uint32_t* table; const uint8_t* state; const unsigned long long* keys; const uint8_t* checks; int hist; int width;
    uint32_t* rec; uint8_t* c_state; unsigned long long* c_keys; uint8_t* c_checks; uint32_t* c_bits; long long* c_actions;
    int* c_model_of;
    const uint8_t* term; const uint8_t* trunc;                 // the reply fork only: the "envs" are child rows, these their done bytes
    // the tree search only (NULL / 0 everywhere else): workgroup e reads row parent_row[e] of the node pool, whose first
    // n_parent rows exist; active[e] = 0 or a row outside them reads as "no candidates" from row e * width, the fallback
    const int* parent_row; const int* active; int n_parent;
};

struct AdvanceArgs {
    uint32_t* rec; uint32_t* tree; int width; int expansions; int t; const uint32_t* table; const int* model_of; int K;
    const float* vl; const float* rewards; const uint8_t* term; const uint8_t* trunc; const unsigned long long* step_err;
    long long* actions; int* parent_row; int* active; int* pv; int* stats; int* err; int n;
};

struct ChooseArgs {
    uint32_t* rec; int width; const uint32_t* table; const int* model_of; int K; const float* vl; const float* rewards;
    const uint8_t* term; const uint8_t* trunc; const unsigned long long* c_err; long long* actions; int* stats; int* err; int n;
    // the reply search only: the children's reply records and what the grandchild step and forward wrote
    uint32_t* r_rec; int rwidth; const float* g_vl; const float* g_rewards; const uint8_t* g_term; const uint8_t* g_trunc;
    const unsigned long long* g_err;
};

// the reply width of model m: word 3 of a row that is on; a word outside [0, 8] reads as 0
__device__ __forceinline__ int la_reply_width(const uint32_t* table, int m, int K) {
    float pw;
    int skip;
    if (la_controls(table, m, K, &pw, &skip) <= 0) return 0;
    const int r = (int)table[(size_t)m * kLaTableWords + 3];
    return r >= 0 && r <= kLaMaxWidth ? r : 0;
}

// kReply = false: the envs fork into their children.  kReply = true: the "envs" are the child rows after their step -- a done
// child is inactive, the width is the reply width of the child's model, skip_plies plays no part, and the action of an unused
// or inactive slot is the lowest legal action of the row's own mask (there is no sampled action to fall back on).
template <bool kReply>
__global__ __launch_bounds__(kLaThreads) void lookahead_fork_kernel(ForkArgs a) {
    __shared__ float row[kPlyA];
    __shared__ uint32_t msk[kPlyWords];
    __shared__ float red[kLaWaves];
    __shared__ int red_i[kLaWaves];
    __shared__ int s_cand[kLaMaxWidth];
    __shared__ float s_prior[kLaMaxWidth];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int width = a.width, W = la_words(width);
    int src = e;                                               // the row this workgroup reads; it writes rows e * width + j
    bool tree = false, off = false;
    if constexpr (kReply) {
        if (a.parent_row) {                                    // the tree search: the parent is a row of the node pool
            const int p = a.parent_row[e];
            tree = true;
            off = a.active[e] == 0 || p < 0 || p >= a.n_parent;
            src = off ? e * width : p;                         // (row e * width of expansion 0 lies below n_parent >= N * width)
        }
    }
    const uint32_t* lw = a.legal + (size_t)src * kPlyWords;
    const int m = a.model_of[src];
    const uint32_t ply = a.state ? *reinterpret_cast<const uint32_t*>(a.state + (size_t)src * kStateBytes + kPlyByte) : UINT_MAX;
    int want;                                                  // (uniform over the workgroup, as every branch below)
    if constexpr (kReply) {
        if (tree) {                                            // the width of the model, not its reply width
            float pw;
            int skip;
            want = (off || (a.term[src] | a.trunc[src])) ? 0 : min(la_controls(a.table, m, a.K, &pw, &skip), width);
        } else {
            want = (a.term[e] | a.trunc[e]) ? 0 : min(la_reply_width(a.table, m, a.K), width);
        }
    } else {
        float pw;
        int skip;
        want = min(la_controls(a.table, m, a.K, &pw, &skip), width);
        if (ply < (uint32_t)skip) want = 0;
    }

    int n_cand = 0;
    if (want > 0) {
        for (int w = tid; w < kPlyWords; w += kLaThreads) msk[w] = mask_word(lw, w);
        const PolicyRowHead h = policy_stage_legal<kLaThreads>(a.logits, a.logits_bf16, (size_t)src * kPlyA, msk, kPlyWords, row);
        const float mx = ka_block_max<kLaThreads>(h.mx, red);  // (a NaN is passed over)
        float s = 0.f;
        policy_for_legal<kLaThreads>(msk, kPlyWords, [&](int j) {
            const float v = row[j];
            if (v == v) s += expf(v - mx);                     // (a NaN logit weighs nothing; -inf gives 0)
        });
        s = ka_block_sum<kLaThreads>(s, red);
        // round r takes the first action behind round r - 1's winner in the candidate order
        float prev_v = INFINITY;
        int prev_i = -1;
        for (int r = 0; r < want; ++r) {
            float bv;
            const int bi = policy_next<kLaThreads, false>(row, msk, kPlyWords, prev_v, prev_i, red, red_i, &bv);
            if (bi == INT_MAX) break;                          // nothing behind the last winner
            if (tid == 0) { s_cand[r] = bi; s_prior[r] = expf(bv - mx) / s; }
            prev_v = bv; prev_i = bi;
            n_cand = r + 1;
        }
    }
    __syncthreads();                                           // s_cand, s_prior

    long long sampled;
    if constexpr (kReply) {                                    // a block min over the first set bits
        int lo = INT_MAX;
        for (int w = tid; w < kPlyWords; w += kLaThreads) {
            const uint32_t mw = mask_word(lw, w);
            if (mw) lo = min(lo, (w << 5) + __builtin_ctz(mw));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
        if (lane == 0) red_i[wave] = lo;
        __syncthreads();
        for (int w = 0; w < kLaWaves; ++w) lo = min(lo, red_i[w]);
        sampled = lo == INT_MAX ? 0 : lo;
    } else {
        sampled = a.actions[e];
    }
    if (tid < W) {
        const int r = tid >= kLaCand ? (tid - kLaCand) % width : 0, part = tid >= kLaCand ? (tid - kLaCand) / width : -1;
        uint32_t word = 0u;
        if (tid == kLaFlags) word = n_cand > 0 ? 1u : 0u;
        else if (tid == kLaNCand) word = (uint32_t)n_cand;
        else if (tid == kLaAction) word = (uint32_t)(int)(sampled < -1 ? -1 : sampled > kPlyA ? kPlyA : sampled);
        else if (part == 0) word = (uint32_t)(r < n_cand ? s_cand[r] : -1);
        else if (part == 1) word = __float_as_uint(r < n_cand ? s_prior[r] : 0.f);
        a.rec[(size_t)e * W + tid] = word;
    }
    if (!a.c_state) return;                                    // candidates and priors only

    // ---- the child rows e * width + j: the row's state and mask for every slot, entries [0, ply) of its history for the
    // slots in use
    const int hist = a.hist;
    const size_t c0 = (size_t)e * width;
    const PlyRow parent{a.state + (size_t)src * kStateBytes, lw, a.keys + (size_t)src * hist, a.checks + (size_t)src * hist};
    ply_fork_rows<kLaThreads>(PlyRows{a.c_state + c0 * kStateBytes, a.c_bits + c0 * kPlyWords, a.c_keys + c0 * hist,
                                      a.c_checks + c0 * hist},
                              width, n_cand, hist, (int)min(ply, (uint32_t)hist), [&](int) { return parent; });
    if (tid < width) {
        const size_t c = c0 + tid;
        const bool used = tid < n_cand;
        a.c_actions[c] = used ? (long long)s_cand[tid] : sampled;
        a.c_model_of[c] = used ? m : -1;
    }
}

// one thread per env: at most eight children each, and with kReplies at most eight grandchildren behind each of them
template <bool kReplies>
__global__ __launch_bounds__(kLaThreads) void lookahead_choose_kernel(ChooseArgs a) {
    const int e = blockIdx.x * kLaThreads + threadIdx.x, lane = threadIdx.x & 63;
    const int width = a.width, W = la_words(width);
    // a refused child step moved no child: its outputs are the unchanged positions, so nothing is chosen from them
    const bool held_c = a.c_err && (a.c_err[0] | a.c_err[1]) != 0ull;
    const bool held_g = kReplies && a.g_err && (a.g_err[0] | a.g_err[1]) != 0ull;
    const bool held = held_c || held_g;
    bool searched = false, changed = false, won = false, bad = false, replied = false;
    if (e < a.n && !held) {
        uint32_t* rec = a.rec + (size_t)e * W;
        if (rec[kLaFlags] & 1u) {
            const int n_cand = min(max((int)rec[kLaNCand], 1), width);
            float pw;
            int skip;
            la_controls(a.table, a.model_of[e], a.K, &pw, &skip);
            int best = 0, best1 = 0;
            float bu = 0.f, bu1 = 0.f;
            for (int j = 0; j < n_cand; ++j) {
                const size_t c = (size_t)e * width + j;
                const bool done = (a.term[c] | a.trunc[c]) != 0;
                float q;
                if (done) {
                    q = a.rewards[c];
                } else {
                    bool b;
                    q = la_loss_minus_win(a.vl, c, &b);        // the child's side to move loses = the mover wins
                    if (b) { bad = true; q = -INFINITY; }
                }
                const float prior = __uint_as_float(rec[kLaCand + width + j]);
                if constexpr (kReplies) {
                    const float u1 = pw > 0.f ? q + pw * prior : q;
                    if (j == 0 || u1 > bu1) { bu1 = u1; best1 = j; }
                    const int R = a.rwidth;
                    uint32_t* rr = a.r_rec + c * la_words(R);
                    if (!done && (rr[kLaFlags] & 1u)) {        // a live child with replies: the worst of them for the mover
                        const int n_rep = min(max((int)rr[kLaNCand], 1), R);
                        int bk = 0;
                        float mn = 0.f;
                        for (int k = 0; k < n_rep; ++k) {
                            const size_t g = c * R + k;
                            float v;
                            if (a.g_term[g] | a.g_trunc[g]) {
                                v = 0.f - a.g_rewards[g];      // the env's reward is for the reply's mover (0 - 0 = +0)
                            } else {
                                bool b;
                                v = 0.f - la_loss_minus_win(a.g_vl, g, &b);       // seen by the root mover again
                                if (b) { bad = true; v = -INFINITY; }
                            }
                            rr[kLaCand + 2 * R + k] = __float_as_uint(v);
                            if (k == 0 || v < mn) { mn = v; bk = k; }             // (ties keep the lower slot)
                        }
                        rr[kLaSlot] = (uint32_t)bk;
                        rr[kLaAction] = rr[kLaCand + bk];
                        q = mn;
                    }
                }
                rec[kLaCand + 2 * width + j] = __float_as_uint(q);
                const float u = pw > 0.f ? q + pw * prior : q;
                if (j == 0 || u > bu) { bu = u; best = j; }    // (ties keep the lower slot)
            }
            const size_t cb = (size_t)e * width + best;
            const int act = (int)rec[kLaCand + best];
            changed = (long long)act != a.actions[e];
            won = a.term[cb] && a.rewards[cb] > 0.f;
            searched = true;
            replied = kReplies && best != best1;
            rec[kLaSlot] = (uint32_t)best;
            rec[kLaAction] = (uint32_t)act;
            rec[kLaFlags] = 1u | ((uint32_t)changed << 1) | ((uint32_t)won << 2) | ((uint32_t)replied << 3);
            a.actions[e] = act;
        }
    }
    const int ns = __popcll(__ballot(searched)), nc = __popcll(__ballot(changed)), nw = __popcll(__ballot(won));
    const int nr = __popcll(__ballot(replied));
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
        if (ns) atomicAdd(&a.stats[0], ns);
        if (nc) atomicAdd(&a.stats[1], nc);
        if (nw) atomicAdd(&a.stats[2], nw);
        if (nr) atomicAdd(&a.stats[3], nr);
        if (any_bad) atomicOr(&a.err[0], 1);
        if (held && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.err[0], (held_c ? 2 : 0) | (held_g ? 4 : 0));
    }
}

// ---- tree search: best-first minimax over `expansions` forks of `width` rows per env (the header above ka_search_words in
// include/keisei_amd.h states the semantics).  Node (t, j) of env e is local node t * width + j and row (t * N + e) * width + j
// of the node pool; record (t, e) is row t * N + e of the records.  The tree of an env, E + 2 E width words:
//   parent[E]  the local node expansion t forked (-1: expansion 0, or an expansion that did not run)
//   val[E * width]  fp32, the backed-up value of every node for the player who moved into it
//   by[E * width]   the expansion that forked the node, -1 = never
constexpr int kLaMaxExpansions = 16, kSearchStatsWords = 5;

__host__ __device__ constexpr int search_tree_words(int width, int expansions) { return expansions + 2 * expansions * width; }

// the expansions of model m: word 3 of its row, outside [1, 16] reads as 1
__device__ __forceinline__ int la_expansions(const uint32_t* table, int m, int K) {
    if (m < 0 || m >= K) return 1;
    const int x = (int)table[(size_t)m * kLaTableWords + 3];
    return x >= 1 && x <= kLaMaxExpansions ? x : 1;
}

// u of a root candidate, the expression of lookahead_choose_kernel
__device__ __forceinline__ float la_u(float q, float pw, float prior) { return pw > 0.f ? q + pw * prior : q; }

// one thread per env, after the forward of expansion t: the leaf q of the new nodes, the backup from the forked node to the
// root, the principal leaf for expansion t + 1, and behind the last expansion the choice
__global__ __launch_bounds__(kLaThreads) void search_advance_kernel(AdvanceArgs a) {
    const int e = blockIdx.x * kLaThreads + threadIdx.x, lane = threadIdx.x & 63;
    const int width = a.width, W = la_words(width), E = a.expansions, t = a.t, N = a.n;
    bool held = false;                                         // a refused step of any expansion so far moved no row
    for (int x = 0; x <= t; ++x) held |= (a.step_err[2 * x] | a.step_err[2 * x + 1]) != 0ull;
    const bool last = t == E - 1;
    bool ran = false, bad = false, searched = false, changed = false, won = false, deepened = false;
    if (e < N) {
        uint32_t* tree = a.tree + (size_t)e * search_tree_words(width, E);
        int* parent = reinterpret_cast<int*>(tree);
        float* val = reinterpret_cast<float*>(tree + E);
        int* by = reinterpret_cast<int*>(tree + E + E * width);
        auto rec_of = [&](int x) { return a.rec + ((size_t)x * N + e) * W; };
        auto row_of = [&](int node) { return ((size_t)(node / width) * N + e) * width + node % width; };
        auto done_at = [&](size_t c) { return (a.term[c] | a.trunc[c]) != 0; };
        auto cands_of = [&](int x) { const uint32_t* r = rec_of(x); return (r[kLaFlags] & 1u) ? min(max((int)r[kLaNCand], 1), width) : 0; };
        uint32_t* rec0 = rec_of(0);
        uint32_t* rect = rec_of(t);
        const int m = a.model_of[e];
        float pw;
        int skip;
        la_controls(a.table, m, a.K, &pw, &skip);
        const int Em = min(la_expansions(a.table, m, a.K), E);
        const bool root = !held && (rec0[kLaFlags] & 1u) != 0;
        if (t == 0)
            for (int x = 0; x < E; ++x) parent[x] = -1;
        // expansion t ran for this env: the root's fork found a candidate, or the launch before this one chose a leaf
        ran = root && (t == 0 || (a.active[e] != 0 && parent[t] >= 0));
        const int n_new = ran ? cands_of(t) : 0;
        for (int j = 0; j < width; ++j) {                      // ---- the leaf q of the new nodes
            float q = 0.f;
            if (j < n_new) {
                const size_t c = row_of(t * width + j);
                if (done_at(c)) {
                    q = a.rewards[c];
                } else {
                    bool b;
                    q = la_loss_minus_win(a.vl, c, &b);        // the node's side to move loses = its mover wins
                    if (b) { bad = true; q = -INFINITY; }
                }
                rect[kLaCand + 2 * width + j] = __float_as_uint(q);
            }
            val[t * width + j] = q;
            by[t * width + j] = -1;
        }
        if (n_new > 0) {                                  // ---- the backup: from the forked node to the root
            int x = t;                                         // the expansion whose children changed
            for (int level = 0; level < kLaMaxExpansions; ++level) {
                uint32_t* r = rec_of(x);
                const int n = cands_of(x);
                int bk = 0;
                float mx = 0.f;
                if (x == 0) {                                  // the root orders by u
                    for (int k = 0; k < n; ++k) {
                        const float u = la_u(val[k], pw, __uint_as_float(r[kLaCand + width + k]));
                        if (k == 0 || u > mx) { mx = u; bk = k; }
                    }
                } else {
                    for (int k = 0; k < n; ++k) {
                        const float v = val[x * width + k];
                        if (k == 0 || v > mx) { mx = v; bk = k; }              // (ties keep the lower slot)
                    }
                }
                r[kLaSlot] = (uint32_t)bk;
                r[kLaAction] = r[kLaCand + bk];
                if (x == 0) break;
                const int p = parent[x];
                if (p < 0 || p >= x * width) break;            // (never: a forked node lies in an earlier expansion)
                val[p] = 0.f - mx;
                x = p / width;
            }
        }
        // ---- the principal leaf: the node expansion t + 1 forks
        int next = -1;
        if (root && t + 1 < Em) {
            int node = (int)rec0[kLaSlot] < cands_of(0) ? (int)rec0[kLaSlot] : 0;
            for (int level = 0; level < kLaMaxExpansions; ++level) {
                if (done_at(row_of(node))) break;              // the game ends on the line: the search is finished
                const int x = by[node];
                if (x < 0 || x > t) { next = node; break; }    // never forked: the leaf
                const int n = cands_of(x);
                if (n == 0) break;                             // forked without a candidate: finished
                const int k = (int)rec_of(x)[kLaSlot];
                node = x * width + (k >= 0 && k < n ? k : 0);
            }
        }
        if (next >= 0) {
            by[next] = t + 1;
            parent[t + 1] = next;
        }
        a.parent_row[e] = next >= 0 ? (int)row_of(next) : -1;
        a.active[e] = next >= 0;
        if (last) {                                            // ---- the choice
            int* pv = a.pv + (size_t)e * E;
            for (int x = 0; x < E; ++x) pv[x] = -1;
            if (root) {
                const int n = cands_of(0);
                const int best = (int)rec0[kLaSlot] < n ? (int)rec0[kLaSlot] : 0;
                int best1 = 0;
                float bu1 = 0.f;
                for (int k = 0; k < n; ++k) {                  // the one-ply choice: the same arg-max over the leaf q
                    const float u1 = la_u(__uint_as_float(rec0[kLaCand + 2 * width + k]), pw, __uint_as_float(rec0[kLaCand + width + k]));
                    if (k == 0 || u1 > bu1) { bu1 = u1; best1 = k; }
                }
                const size_t cb = row_of(best);
                const int act = (int)rec0[kLaCand + best];
                changed = (long long)act != a.actions[e];
                won = a.term[cb] && a.rewards[cb] > 0.f;
                searched = true;
                deepened = best != best1;
                rec0[kLaAction] = (uint32_t)act;
                rec0[kLaFlags] = 1u | ((uint32_t)changed << 1) | ((uint32_t)won << 2) | ((uint32_t)deepened << 3);
                a.actions[e] = act;
                int node = best, len = 0;
                pv[len++] = act;
                while (len < E && !done_at(row_of(node))) {    // the first-maximum children down the line
                    const int x = by[node];
                    if (x < 0 || x > t) break;
                    const int n2 = cands_of(x);
                    if (n2 == 0) break;
                    const uint32_t* r = rec_of(x);
                    const int k = (int)r[kLaSlot] < n2 ? (int)r[kLaSlot] : 0;
                    pv[len++] = (int)r[kLaCand + k];
                    node = x * width + k;
                }
            }
        }
    }
    const int nx = __popcll(__ballot(ran));
    const bool any_bad = __ballot(bad) != 0ull;
    const int ns = __popcll(__ballot(searched)), nc = __popcll(__ballot(changed)), nw = __popcll(__ballot(won));
    const int nd = __popcll(__ballot(deepened));
    if (lane == 0) {
        if (ns) atomicAdd(&a.stats[0], ns);
        if (nc) atomicAdd(&a.stats[1], nc);
        if (nw) atomicAdd(&a.stats[2], nw);
        if (nd) atomicAdd(&a.stats[3], nd);
        if (nx) atomicAdd(&a.stats[4], nx);
        if (any_bad) atomicOr(&a.err[0], 1);
        if (held && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.err[0], 2);
    }
}

}  // namespace

extern "C" int ka_lookahead_words(int which, int width) {
    if (width < 0 || width > kLaMaxWidth) return -1;
    return which == 0 ? la_words(width) : which == 1 ? kLaTableWords : which == 2 ? kLaStatsWords : which == 3 ? kLaMaxWidth :
           which == 4 ? kLaMaxWidth /* reply width */ : which == 5 ? kLaMaxWidth * kLaMaxWidth /* grandchildren per env */ : -1;
}

extern "C" int ka_lookahead_fork(const void* logits, int logits_bf16, const void* legal, int legal_words, const long long* actions,
                                 const int* model_of, int K, const void* table, const void* state, const void* keys,
                                 const void* checks, int max_ply, int width, void* records, void* child_state, void* child_keys,
                                 void* child_checks, void* child_mask_bits, long long* child_actions, int* child_model_of, int N,
                                 int A, void* stream) {
    KA_REQUIRE(logits && legal && actions && model_of && table && records && N > 0, "lookahead_fork: null tensor");
    KA_REQUIRE_PLY_SPACE("lookahead_fork", A, legal_words);
    KA_REQUIRE(width >= 1 && width <= kLaMaxWidth, "lookahead_fork: width must lie in [1, %d], got %d", kLaMaxWidth, width);
    KA_REQUIRE(K >= 1, "lookahead_fork: the controls table needs at least one row, got K = %d", K);
    const bool rows = state || keys || checks || child_state || child_keys || child_checks || child_mask_bits || child_actions ||
                      child_model_of;
    KA_REQUIRE(!rows || (state && keys && checks && child_state && child_keys && child_checks && child_mask_bits &&
                         child_actions && child_model_of),
               "lookahead_fork: the env rows and the child rows are all given or all NULL");
    KA_REQUIRE_MAX_PLY("lookahead_fork", max_ply);
    KA_REQUIRE((long long)N * width <= INT_MAX, "lookahead_fork: %d envs of width %d are too many child rows", N, width);
    KA_REQUIRE(ka_aligned(logits_bf16 ? 2 : 4, {logits}) &&
               ka_aligned(16, {legal, state, keys, checks, child_state, child_keys, child_checks, child_mask_bits}) &&
               ka_aligned(8, {actions, child_actions}) && ka_aligned(4, {model_of, table, records, child_model_of}),
               "lookahead_fork: state, history and mask rows are 16-byte aligned, every other tensor to its element size");
    ForkArgs a{logits, logits_bf16, static_cast<const uint32_t*>(legal), actions, model_of, K, static_cast<const uint32_t*>(table),
               static_cast<const uint8_t*>(state), static_cast<const unsigned long long*>(keys),
               static_cast<const uint8_t*>(checks), max_ply > 0 ? max_ply : 1, width, static_cast<uint32_t*>(records),
               static_cast<uint8_t*>(child_state), static_cast<unsigned long long*>(child_keys),
               static_cast<uint8_t*>(child_checks), static_cast<uint32_t*>(child_mask_bits), child_actions, child_model_of,
               nullptr, nullptr};
    hipLaunchKernelGGL(lookahead_fork_kernel<false>, dim3(N), dim3(kLaThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("lookahead_fork");
}

extern "C" int ka_lookahead_choose(void* records, int width, const void* table, const int* model_of, int K,
                                   const float* child_vlogits, const float* child_rewards, const void* child_terminated,
                                   const void* child_truncated, const void* child_err, long long* actions, int* stats, int* err,
                                   int N, void* stream) {
    KA_REQUIRE(records && table && model_of && child_vlogits && child_rewards && child_terminated && child_truncated && actions &&
               stats && err && N > 0, "lookahead_choose: null tensor");
    KA_REQUIRE(width >= 1 && width <= kLaMaxWidth, "lookahead_choose: width must lie in [1, %d], got %d", kLaMaxWidth, width);
    KA_REQUIRE(K >= 1, "lookahead_choose: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)table % 4 == 0 && (uintptr_t)model_of % 4 == 0 &&
               (uintptr_t)child_vlogits % 4 == 0 && (uintptr_t)child_rewards % 4 == 0 && (uintptr_t)child_err % 8 == 0 &&
               (uintptr_t)actions % 8 == 0 && (uintptr_t)stats % 4 == 0 && (uintptr_t)err % 4 == 0,
               "lookahead_choose: actions and the child error words are 8-byte aligned, every other tensor to its element size");
    ChooseArgs a{static_cast<uint32_t*>(records), width, static_cast<const uint32_t*>(table), model_of, K, child_vlogits,
                 child_rewards, static_cast<const uint8_t*>(child_terminated), static_cast<const uint8_t*>(child_truncated),
                 static_cast<const unsigned long long*>(child_err), actions, stats, err, N,
                 nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(lookahead_choose_kernel<false>, dim3((N + kLaThreads - 1) / kLaThreads), dim3(kLaThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("lookahead_choose");
}

extern "C" int ka_lookahead_fork_replies(const void* child_logits, int logits_bf16, const void* child_mask_bits, int legal_words,
                                         const int* child_model_of, int K, const void* table, const void* child_state,
                                         const void* child_keys, const void* child_checks, const void* child_terminated,
                                         const void* child_truncated, int max_ply, int reply_width, void* reply_records,
                                         void* grand_state, void* grand_keys, void* grand_checks, void* grand_mask_bits,
                                         long long* grand_actions, int* grand_model_of, int M, int A, void* stream) {
    KA_REQUIRE(child_logits && child_mask_bits && child_model_of && table && child_state && child_keys && child_checks &&
               child_terminated && child_truncated && reply_records && grand_state && grand_keys && grand_checks &&
               grand_mask_bits && grand_actions && grand_model_of && M > 0, "lookahead_fork_replies: null tensor");
    KA_REQUIRE_PLY_SPACE("lookahead_fork_replies", A, legal_words);
    KA_REQUIRE(reply_width >= 1 && reply_width <= kLaMaxWidth, "lookahead_fork_replies: reply_width must lie in [1, %d], got %d",
               kLaMaxWidth, reply_width);
    KA_REQUIRE(K >= 1, "lookahead_fork_replies: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE_MAX_PLY("lookahead_fork_replies", max_ply);
    KA_REQUIRE((long long)M * reply_width <= INT_MAX, "lookahead_fork_replies: %d children of reply width %d are too many rows", M,
               reply_width);
    KA_REQUIRE(ka_aligned(logits_bf16 ? 2 : 4, {child_logits}) &&
               ka_aligned(16, {child_mask_bits, child_state, child_keys, child_checks, grand_state, grand_keys, grand_checks,
                               grand_mask_bits}) &&
               ka_aligned(8, {grand_actions}) && ka_aligned(4, {child_model_of, table, reply_records, grand_model_of}),
               "lookahead_fork_replies: state, history and mask rows are 16-byte aligned, every other tensor to its element size");
    ForkArgs a{child_logits, logits_bf16, static_cast<const uint32_t*>(child_mask_bits), nullptr, child_model_of, K,
               static_cast<const uint32_t*>(table), static_cast<const uint8_t*>(child_state),
               static_cast<const unsigned long long*>(child_keys), static_cast<const uint8_t*>(child_checks),
               max_ply > 0 ? max_ply : 1, reply_width, static_cast<uint32_t*>(reply_records), static_cast<uint8_t*>(grand_state),
               static_cast<unsigned long long*>(grand_keys), static_cast<uint8_t*>(grand_checks),
               static_cast<uint32_t*>(grand_mask_bits), grand_actions, grand_model_of,
               static_cast<const uint8_t*>(child_terminated), static_cast<const uint8_t*>(child_truncated)};
    hipLaunchKernelGGL(lookahead_fork_kernel<true>, dim3(M), dim3(kLaThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("lookahead_fork_replies");
}

extern "C" int ka_lookahead_choose_replies(void* records, int width, void* reply_records, int reply_width, const void* table,
                                           const int* model_of, int K, const float* child_vlogits, const float* child_rewards,
                                           const void* child_terminated, const void* child_truncated, const void* child_err,
                                           const float* grand_vlogits, const float* grand_rewards, const void* grand_terminated,
                                           const void* grand_truncated, const void* grand_err, long long* actions, int* stats,
                                           int* err, int N, void* stream) {
    KA_REQUIRE(records && reply_records && table && model_of && child_vlogits && child_rewards && child_terminated &&
               child_truncated && grand_vlogits && grand_rewards && grand_terminated && grand_truncated && actions && stats &&
               err && N > 0, "lookahead_choose_replies: null tensor");
    KA_REQUIRE(width >= 1 && width <= kLaMaxWidth, "lookahead_choose_replies: width must lie in [1, %d], got %d", kLaMaxWidth, width);
    KA_REQUIRE(reply_width >= 1 && reply_width <= kLaMaxWidth, "lookahead_choose_replies: reply_width must lie in [1, %d], got %d",
               kLaMaxWidth, reply_width);
    KA_REQUIRE(K >= 1, "lookahead_choose_replies: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE((long long)N * width * reply_width <= INT_MAX, "lookahead_choose_replies: too many grandchild rows");
    KA_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)reply_records % 4 == 0 && (uintptr_t)table % 4 == 0 &&
               (uintptr_t)model_of % 4 == 0 && (uintptr_t)child_vlogits % 4 == 0 && (uintptr_t)child_rewards % 4 == 0 &&
               (uintptr_t)child_err % 8 == 0 && (uintptr_t)grand_vlogits % 4 == 0 && (uintptr_t)grand_rewards % 4 == 0 &&
               (uintptr_t)grand_err % 8 == 0 && (uintptr_t)actions % 8 == 0 && (uintptr_t)stats % 4 == 0 && (uintptr_t)err % 4 == 0,
               "lookahead_choose_replies: actions and the error words are 8-byte aligned, every other tensor to its element size");
    ChooseArgs a{static_cast<uint32_t*>(records), width, static_cast<const uint32_t*>(table), model_of, K, child_vlogits,
                 child_rewards, static_cast<const uint8_t*>(child_terminated), static_cast<const uint8_t*>(child_truncated),
                 static_cast<const unsigned long long*>(child_err), actions, stats, err, N,
                 static_cast<uint32_t*>(reply_records), reply_width, grand_vlogits, grand_rewards,
                 static_cast<const uint8_t*>(grand_terminated), static_cast<const uint8_t*>(grand_truncated),
                 static_cast<const unsigned long long*>(grand_err)};
    hipLaunchKernelGGL(lookahead_choose_kernel<true>, dim3((N + kLaThreads - 1) / kLaThreads), dim3(kLaThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("lookahead_choose_replies");
}

extern "C" int ka_search_words(int which, int width, int expansions) {
    if (width < 0 || width > kLaMaxWidth || expansions < 0 || expansions > kLaMaxExpansions) return -1;
    return which == 0 ? la_words(width) : which == 1 ? search_tree_words(width, expansions) : which == 2 ? kSearchStatsWords :
           which == 3 ? kLaMaxWidth : which == 4 ? kLaMaxExpansions : which == 5 ? kLaTableWords : -1;
}

extern "C" int ka_search_expand(const void* pool_logits, int logits_bf16, const void* pool_mask_bits, int legal_words,
                                const int* pool_model_of, int K, const void* table, const void* pool_state,
                                const void* pool_keys, const void* pool_checks, const void* pool_terminated,
                                const void* pool_truncated, int max_ply, int width, int t, const int* parent_row,
                                const int* active, void* records, void* node_state, void* node_keys, void* node_checks,
                                void* node_mask_bits, long long* node_actions, int* node_model_of, int N, int A, void* stream) {
    KA_REQUIRE(pool_logits && pool_mask_bits && pool_model_of && table && pool_state && pool_keys && pool_checks &&
               pool_terminated && pool_truncated && parent_row && active && records && node_state && node_keys && node_checks &&
               node_mask_bits && node_actions && node_model_of && N > 0, "search_expand: null tensor");
    KA_REQUIRE_PLY_SPACE("search_expand", A, legal_words);
    KA_REQUIRE(width >= 1 && width <= kLaMaxWidth, "search_expand: width must lie in [1, %d], got %d", kLaMaxWidth, width);
    KA_REQUIRE(t >= 1 && t < kPoolMaxSlices, "search_expand: the expansion must lie in [1, %d), got %d", kPoolMaxSlices, t);
    KA_REQUIRE(K >= 1, "search_expand: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE_MAX_PLY("search_expand", max_ply);
    KA_REQUIRE((long long)N * width * (t + 1) <= INT_MAX, "search_expand: %d envs of width %d are too many rows at expansion %d", N,
               width, t);
    const size_t below = (size_t)t * N * width;                // the rows of the expansions before this one
    KA_REQUIRE(static_cast<const uint8_t*>(node_state) == static_cast<const uint8_t*>(pool_state) + below * kStateBytes &&
               static_cast<const int*>(node_model_of) == pool_model_of + below,
               "search_expand: the rows written are slice %d of the pool: they start %zu rows behind it", t, below);
    KA_REQUIRE(ka_aligned(logits_bf16 ? 2 : 4, {pool_logits}) &&
               ka_aligned(16, {pool_mask_bits, pool_state, pool_keys, pool_checks, node_state, node_mask_bits}) &&
               ka_aligned(8, {node_actions}) &&
               ka_aligned(4, {pool_model_of, table, records, parent_row, active, node_model_of}),
               "search_expand: state, history and mask rows are 16-byte aligned, every other tensor to its element size");
    // a slice of the pool starts a whole number of history rows behind it: aligned to the pieces its rows are copied in
    const int hist = max_ply > 0 ? max_ply : 1;
    KA_REQUIRE((uintptr_t)node_keys % (hist % 2 == 0 ? 16 : 8) == 0 &&
               (uintptr_t)node_checks % (hist % 16 == 0 ? 16 : hist % 4 == 0 ? 4 : 1) == 0,
               "search_expand: the history rows written are aligned to the pieces rows of %d entries are copied in", hist);
    ForkArgs a{pool_logits, logits_bf16, static_cast<const uint32_t*>(pool_mask_bits), nullptr, pool_model_of, K,
               static_cast<const uint32_t*>(table), static_cast<const uint8_t*>(pool_state),
               static_cast<const unsigned long long*>(pool_keys), static_cast<const uint8_t*>(pool_checks),
               max_ply > 0 ? max_ply : 1, width, static_cast<uint32_t*>(records), static_cast<uint8_t*>(node_state),
               static_cast<unsigned long long*>(node_keys), static_cast<uint8_t*>(node_checks),
               static_cast<uint32_t*>(node_mask_bits), node_actions, node_model_of,
               static_cast<const uint8_t*>(pool_terminated), static_cast<const uint8_t*>(pool_truncated),
               parent_row, active, (int)below};
    hipLaunchKernelGGL(lookahead_fork_kernel<true>, dim3(N), dim3(kLaThreads), 0, static_cast<hipStream_t>(stream), a);
    return ka_check_launch("search_expand");
}

extern "C" int ka_search_advance(void* records, void* tree, int width, int expansions, int t, const void* table,
                                 const int* model_of, int K, const float* pool_vlogits, const float* pool_rewards,
                                 const void* pool_terminated, const void* pool_truncated, const void* step_err,
                                 long long* actions, int* parent_row, int* active, int* pv, int* stats, int* err, int N,
                                 void* stream) {
    KA_REQUIRE(records && tree && table && model_of && pool_vlogits && pool_rewards && pool_terminated && pool_truncated &&
               step_err && actions && parent_row && active && pv && stats && err && N > 0, "search_advance: null tensor");
    KA_REQUIRE(width >= 1 && width <= kLaMaxWidth, "search_advance: width must lie in [1, %d], got %d", kLaMaxWidth, width);
    KA_REQUIRE(expansions >= 1 && expansions <= kLaMaxExpansions, "search_advance: expansions must lie in [1, %d], got %d",
               kLaMaxExpansions, expansions);
    KA_REQUIRE(t >= 0 && t < expansions, "search_advance: the expansion must lie in [0, %d), got %d", expansions, t);
    KA_REQUIRE(K >= 1, "search_advance: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE((long long)N * width * expansions <= INT_MAX, "search_advance: too many node rows");
    KA_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)tree % 4 == 0 && (uintptr_t)table % 4 == 0 && (uintptr_t)model_of % 4 == 0 &&
               (uintptr_t)pool_vlogits % 4 == 0 && (uintptr_t)pool_rewards % 4 == 0 && (uintptr_t)step_err % 8 == 0 &&
               (uintptr_t)actions % 8 == 0 && (uintptr_t)parent_row % 4 == 0 && (uintptr_t)active % 4 == 0 &&
               (uintptr_t)pv % 4 == 0 && (uintptr_t)stats % 4 == 0 && (uintptr_t)err % 4 == 0,
               "search_advance: actions and the step error words are 8-byte aligned, every other tensor to its element size");
    AdvanceArgs a{static_cast<uint32_t*>(records), static_cast<uint32_t*>(tree), width, expansions, t,
                  static_cast<const uint32_t*>(table), model_of, K, pool_vlogits, pool_rewards,
                  static_cast<const uint8_t*>(pool_terminated), static_cast<const uint8_t*>(pool_truncated),
                  static_cast<const unsigned long long*>(step_err), actions, parent_row, active, pv, stats, err, N};
    hipLaunchKernelGGL(search_advance_kernel, dim3((N + kLaThreads - 1) / kLaThreads), dim3(kLaThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("search_advance");
}
