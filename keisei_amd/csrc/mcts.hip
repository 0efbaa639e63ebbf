// Visit-count (PUCT) search in the device ply.  The tree search of csrc/lookahead.hip spends every fork on the leaf of the
// current principal variation and backs up by max and negation; this one spreads `simulations` forks of `width` rows per env
// by Q + c P sqrt(N) / (1 + n), backs values up as means and plays the most visited root candidate.  Everything that moves
// rows is what the tree search uses, unchanged: the node pool of complete env rows, ka_lookahead_fork for the root,
// ka_search_expand for a named leaf, ka_shogi_env_step and the grouped forward over a slice.  New is the tree policy:
//
//   ka_mcts_advance     one thread per env, after the forward of simulation t: the leaf q of the new nodes, the backup of
//                       simulation t, the selection for simulation t + 1 (parent_row / active for ka_search_expand), and
//                       behind the last launch the choice, the flags, the principal variation and the counters
//   ka_mcts_advance_explore   the same kernel with an exploration table (csrc/mcts_explore.h): where the env's game ply lies
//                       below its model's sample_plies the played move is drawn in proportion to the root visits
//
// The header above ka_mcts_words in include/keisei_amd.h states the semantics.  Node (t, j) of env e is local node
// t * width + j and row (t * N + e) * width + j of the node pool; record (t, e) is row t * N + e of the records (the
// lookahead's layout, csrc/lookahead_record.h).  The tree of an env, E + 4 E width words for E simulations:
//   parent[E]           the local node simulation t selected (-1: simulation 0, or a simulation that did not run)
//   visits[E * width]   int32 N
//   sum[E * width]      fp32 S, the value sum for the player who moved into the node
//   prior[E * width]    fp32 P, as the fork that created the node wrote it
//   by[E * width]       the simulation that forked the node, -1 = never
// A simulation whose parent has by[parent] == t forked it; any other simulation that ran was a revisit.
//
// One thread per env: the tree of an env is at most 64 * 8 nodes of 16 bytes walked from the root down and back up, every
// step depending on the one before, and the order of the fp32 adds into S is part of the contract -- there is nothing in it
// for a second lane to do.  The launch is bound by the latency of those dependent loads (a few per level, the tree lies in
// L2 between the launches of a ply), not by bandwidth or arithmetic.
#include "mcts_explore.h"

#include <climits>

namespace {

constexpr int kMcThreads = 256;
constexpr int kMcMaxSimulations = 64, kMcStatsWords = 6;
static_assert(kMcMaxSimulations <= kPoolMaxSlices, "ka_search_expand writes every slice of the pool");

__host__ __device__ constexpr int mcts_tree_words(int width, int sims) { return sims + 4 * sims * width; }

struct MctsArgs {
    uint32_t* rec; uint32_t* tree; int width; int sims; int t; const uint32_t* table; const int* model_of; int K;
    const float* vl; const float* rewards; const uint8_t* term; const uint8_t* trunc; const unsigned long long* step_err;
    long long* actions; int* parent_row; int* active; int* pv; int* root_visits; float* root_values; int* stats; int* err; int n;
    // the exploration of ka_mcts_advance_explore; xtable == nullptr is ka_mcts_advance
    const uint32_t* xtable; const long long* seed_dev; const uint8_t* plies; int ply_stride; int* xstats;
};

// the simulations of model m: word 3 of its row, outside [1, 64] reads as 1
__device__ __forceinline__ int mcts_simulations(const uint32_t* table, int m, int K) {
    if (m < 0 || m >= K) return 1;
    const int x = (int)table[(size_t)m * kLaTableWords + 3];
    return x >= 1 && x <= kMcMaxSimulations ? x : 1;
}

__global__ __launch_bounds__(kMcThreads) void mcts_advance_kernel(MctsArgs a) {
    const int e = blockIdx.x * kMcThreads + threadIdx.x, lane = threadIdx.x & 63;
    const int width = a.width, W = la_words(width), E = a.sims, t = a.t, N = a.n;
    bool held = false;                                         // a refused step of any simulation so far moved no row
    for (int x = 0; x <= t; ++x) held |= (a.step_err[2 * x] | a.step_err[2 * x + 1]) != 0ull;
    const bool last = t == E - 1;
    bool ran = false, revisit = false, bad = false, searched = false, changed = false, won = false, deepened = false;
    bool sampled = false, diverged = false;
    if (e < N) {
        uint32_t* tree = a.tree + (size_t)e * mcts_tree_words(width, E);
        int* parent = reinterpret_cast<int*>(tree);
        int* visits = reinterpret_cast<int*>(tree + E);
        float* sum = reinterpret_cast<float*>(tree + E + E * width);
        float* prior = reinterpret_cast<float*>(tree + E + 2 * E * width);
        int* by = reinterpret_cast<int*>(tree + E + 3 * E * width);
        auto rec_of = [&](int x) { return a.rec + ((size_t)x * N + e) * W; };
        auto row_of = [&](int node) { return ((size_t)(node / width) * N + e) * width + node % width; };
        auto done_at = [&](size_t c) { return (a.term[c] | a.trunc[c]) != 0; };
        auto cands_of = [&](int x) { const uint32_t* r = rec_of(x); return (r[kLaFlags] & 1u) ? min(max((int)r[kLaNCand], 1), width) : 0; };
        auto leaf_q = [&](int node) { return __uint_as_float(rec_of(node / width)[kLaCand + 2 * width + node % width]); };
        uint32_t* rec0 = rec_of(0);
        uint32_t* rect = rec_of(t);
        const int m = a.model_of[e];
        float c_puct;
        int skip;
        la_controls(a.table, m, a.K, &c_puct, &skip);
        const int Em = min(mcts_simulations(a.table, m, a.K), E);
        const bool root = !held && (rec0[kLaFlags] & 1u) != 0;
        if (t == 0)
            for (int x = 0; x < E; ++x) parent[x] = -1;
        // simulation t ran for this env: the root's fork found a candidate, or the launch before this one selected a node
        const int leaf = t == 0 ? -1 : parent[t];
        ran = root && (t == 0 || (leaf >= 0 && leaf < t * width));
        const bool forked = ran && (t == 0 || (a.active[e] != 0 && by[leaf] == t));
        const int n_new = forked ? cands_of(t) : 0;
        float v = 0.f;                                         // the first maximum of the new nodes' q (exact)
        for (int j = 0; j < width; ++j) {                      // ---- the leaf q of the new nodes: N = 1, S = q
            float q = 0.f;
            if (j < n_new) {
                const size_t c = row_of(t * width + j);
                if (done_at(c)) {
                    q = a.rewards[c];
                } else {
                    bool b;
                    q = la_loss_minus_win(a.vl, c, &b);        // the node's side to move loses = its mover wins
                    if (b) { bad = true; q = 0.f; }            // no NaN enters a tree; the error word tells
                }
                rect[kLaCand + 2 * width + j] = __float_as_uint(q);
                if (j == 0 || q > v) v = q;
            }
            visits[t * width + j] = j < n_new ? 1 : 0;
            sum[t * width + j] = q;
            prior[t * width + j] = j < n_new ? __uint_as_float(rect[kLaCand + width + j]) : 0.f;
            by[t * width + j] = -1;
        }
        if (ran && t > 0) {                                    // ---- the backup: from the selected node to the root's child
            // a fork with children gives the node 0 - v; a revisit (a done node, a node forked without a candidate, now or
            // before) gives it its own leaf q again; the signs alternate up the path
            revisit = n_new == 0;
            float val = revisit ? leaf_q(leaf) : 0.f - v;
            int node = leaf;
            for (int level = 0; level < kMcMaxSimulations; ++level) {
                visits[node] += 1;
                sum[node] += val;
                const int x = node / width;
                if (x == 0) break;
                const int p = parent[x];
                if (p < 0 || p >= x * width) break;            // (never: a forked node lies in an earlier simulation)
                node = p;
                val = 0.f - val;
            }
        }
        // ---- the selection for simulation t + 1
        int next = -1;
        bool fork_next = false;
        if (root && t + 1 < Em) {
            int x = 0;
            for (int level = 0; level < kMcMaxSimulations; ++level) {
                uint32_t* r = rec_of(x);
                const int n = cands_of(x);                     // (> 0: the root has a candidate, and so has every node descended into)
                int n_par = 0;
                for (int k = 0; k < n; ++k) n_par += visits[x * width + k];
                const float sq = sqrtf((float)n_par);
                int bk = 0;
                float bs = 0.f;
                for (int k = 0; k < n; ++k) {
                    const int nk = visits[x * width + k];
                    float s = sum[x * width + k] / (float)nk;
                    if (c_puct > 0.f) s = s + c_puct * prior[x * width + k] * sq / (float)(1 + nk);
                    if (k == 0 || s > bs) { bs = s; bk = k; }  // (ties keep the lower slot)
                }
                r[kLaSlot] = (uint32_t)bk;
                r[kLaAction] = r[kLaCand + bk];
                next = x * width + bk;
                if (done_at(row_of(next))) break;              // the game ended there: a revisit
                const int bx = by[next];
                if (bx < 0 || bx > t) { fork_next = true; break; }             // never forked and live: the leaf
                if (cands_of(bx) == 0) break;                  // forked without a candidate: a revisit
                x = bx;
            }
        }
        if (next >= 0) parent[t + 1] = next;
        if (fork_next) by[next] = t + 1;
        a.parent_row[e] = fork_next ? (int)row_of(next) : -1;
        a.active[e] = fork_next;
        if (last) {                                            // ---- the choice
            int* pv = a.pv + (size_t)e * E;
            for (int x = 0; x < E; ++x) pv[x] = -1;
            for (int k = 0; k < width; ++k) {
                const int nk = root ? visits[k] : 0;
                a.root_visits[(size_t)e * width + k] = nk;
                a.root_values[(size_t)e * width + k] = nk > 0 ? sum[k] / (float)nk : 0.f;
            }
            if (root) {
                const int n = cands_of(0);
                int best = 0, best1 = 0;
                for (int k = 1; k < n; ++k) {                  // most visits; the one-ply choice: the same arg-max over the leaf q
                    if (visits[k] > visits[best]) best = k;
                    if (leaf_q(k) > leaf_q(best1)) best1 = k;
                }
                int play = best;                               // the played slot: best, or drawn in proportion to the visits
                if (a.xtable) {
                    float eps, alpha;
                    int sample_plies;
                    xp_controls(a.xtable, m, a.K, &eps, &alpha, &sample_plies);
                    const uint32_t ply = *reinterpret_cast<const uint32_t*>(a.plies + (size_t)e * a.ply_stride);
                    if (ply < (uint32_t)sample_plies) {
                        unsigned long long total = 0ull, run = 0ull;
                        for (int k = 0; k < n; ++k) total += (unsigned long long)visits[k];
                        const unsigned long long r0 = xp_draw(xp_stream((unsigned long long)*a.seed_dev, e, kXpChoice), 0);
                        const unsigned long long x = ((r0 >> 32) * total) >> 32;      // in [0, total)
                        for (int k = 0; k < n; ++k) {              // the first slot whose running sum exceeds x
                            run += (unsigned long long)visits[k];
                            if (run > x) { play = k; break; }
                        }
                        sampled = true;
                        diverged = play != best;
                    }
                }
                const size_t cb = row_of(play);
                const int act = (int)rec0[kLaCand + play];
                changed = (long long)act != a.actions[e];
                won = a.term[cb] && a.rewards[cb] > 0.f;
                searched = true;
                deepened = best != best1;
                rec0[kLaSlot] = (uint32_t)play;
                rec0[kLaAction] = (uint32_t)act;
                rec0[kLaFlags] = 1u | ((uint32_t)changed << 1) | ((uint32_t)won << 2) | ((uint32_t)deepened << 3) |
                                 ((uint32_t)sampled << 4) | ((uint32_t)diverged << 5);
                a.actions[e] = act;
                int node = play, len = 0;
                pv[len++] = act;
                while (len < E && !done_at(row_of(node))) {    // the most visited children down the line
                    const int x = by[node];
                    if (x < 0 || x > t) break;
                    const int n2 = cands_of(x);
                    if (n2 == 0) break;
                    int k = 0;
                    for (int j = 1; j < n2; ++j)
                        if (visits[x * width + j] > visits[x * width + k]) k = j;
                    pv[len++] = (int)rec_of(x)[kLaCand + k];
                    node = x * width + k;
                }
            }
        }
    }
    const int nx = __popcll(__ballot(ran)), nr = __popcll(__ballot(revisit));
    const bool any_bad = __ballot(bad) != 0ull;
    const int ns = __popcll(__ballot(searched)), nc = __popcll(__ballot(changed)), nw = __popcll(__ballot(won));
    const int nd = __popcll(__ballot(deepened));
    if (lane == 0) {
        if (ns) atomicAdd(&a.stats[0], ns);
        if (nc) atomicAdd(&a.stats[1], nc);
        if (nw) atomicAdd(&a.stats[2], nw);
        if (nd) atomicAdd(&a.stats[3], nd);
        if (nx) atomicAdd(&a.stats[4], nx);
        if (nr) atomicAdd(&a.stats[5], nr);
        if (any_bad) atomicOr(&a.err[0], 1);
        if (held && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.err[0], 2);
    }
    if (a.xtable && last) {                                    // (wave-uniform: the ballots are whole)
        const int nsm = __popcll(__ballot(sampled)), ndv = __popcll(__ballot(diverged));
        if (lane == 0 && nsm) atomicAdd(&a.xstats[1], nsm);
        if (lane == 0 && ndv) atomicAdd(&a.xstats[2], ndv);
    }
}

}  // namespace

extern "C" int ka_mcts_words(int which, int width, int simulations) {
    if (width < 0 || width > kLaMaxWidth || simulations < 0 || simulations > kMcMaxSimulations) return -1;
    return which == 0 ? la_words(width) : which == 1 ? mcts_tree_words(width, simulations) : which == 2 ? kMcStatsWords :
           which == 3 ? kLaMaxWidth : which == 4 ? kMcMaxSimulations : which == 5 ? kLaTableWords :
           which == 7 ? kXpStatsWords : -1;
}

extern "C" int ka_mcts_advance_explore(void* records, void* tree, int width, int simulations, int t, const void* table,
                                       const int* model_of, int K, const float* pool_vlogits, const float* pool_rewards,
                                       const void* pool_terminated, const void* pool_truncated, const void* step_err,
                                       long long* actions, int* parent_row, int* active, int* pv, int* root_visits,
                                       float* root_values, int* stats, int* err, const void* explore_table,
                                       const long long* seed_dev, const void* plies, int ply_stride, int* explore_stats, int N,
                                       void* stream) {
    KA_REQUIRE(records && tree && table && model_of && pool_vlogits && pool_rewards && pool_terminated && pool_truncated &&
               step_err && actions && parent_row && active && pv && root_visits && root_values && stats && err && N > 0,
               "mcts_advance: null tensor");
    KA_REQUIRE(width >= 1 && width <= kLaMaxWidth, "mcts_advance: width must lie in [1, %d], got %d", kLaMaxWidth, width);
    KA_REQUIRE(simulations >= 1 && simulations <= kMcMaxSimulations, "mcts_advance: simulations must lie in [1, %d], got %d",
               kMcMaxSimulations, simulations);
    KA_REQUIRE(t >= 0 && t < simulations, "mcts_advance: the simulation must lie in [0, %d), got %d", simulations, t);
    KA_REQUIRE(K >= 1, "mcts_advance: the controls table needs at least one row, got K = %d", K);
    KA_REQUIRE((long long)N * width * simulations <= INT_MAX, "mcts_advance: too many node rows");
    KA_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)tree % 4 == 0 && (uintptr_t)table % 4 == 0 && (uintptr_t)model_of % 4 == 0 &&
               (uintptr_t)pool_vlogits % 4 == 0 && (uintptr_t)pool_rewards % 4 == 0 && (uintptr_t)step_err % 8 == 0 &&
               (uintptr_t)actions % 8 == 0 && (uintptr_t)parent_row % 4 == 0 && (uintptr_t)active % 4 == 0 &&
               (uintptr_t)pv % 4 == 0 && (uintptr_t)root_visits % 4 == 0 && (uintptr_t)root_values % 4 == 0 &&
               (uintptr_t)stats % 4 == 0 && (uintptr_t)err % 4 == 0,
               "mcts_advance: actions and the step error words are 8-byte aligned, every other tensor to its element size");
    if (explore_table) {
        KA_REQUIRE(seed_dev && plies && explore_stats, "mcts_advance: an exploration table needs the seed, the game plies and its counters");
        KA_REQUIRE(ply_stride >= 4, "mcts_advance: ply_stride must be at least 4 bytes, got %d", ply_stride);
        KA_REQUIRE((uintptr_t)explore_table % 4 == 0 && (uintptr_t)seed_dev % 8 == 0 && (uintptr_t)plies % 4 == 0 &&
                   ply_stride % 4 == 0 && (uintptr_t)explore_stats % 4 == 0,
                   "mcts_advance: the seed is 8-byte aligned, the exploration table, the game plies and the counters to 4 bytes");
    }
    MctsArgs a{static_cast<uint32_t*>(records), static_cast<uint32_t*>(tree), width, simulations, t,
               static_cast<const uint32_t*>(table), model_of, K, pool_vlogits, pool_rewards,
               static_cast<const uint8_t*>(pool_terminated), static_cast<const uint8_t*>(pool_truncated),
               static_cast<const unsigned long long*>(step_err), actions, parent_row, active, pv, root_visits, root_values,
               stats, err, N, static_cast<const uint32_t*>(explore_table), seed_dev, static_cast<const uint8_t*>(plies),
               ply_stride, explore_stats};
    hipLaunchKernelGGL(mcts_advance_kernel, dim3((N + kMcThreads - 1) / kMcThreads), dim3(kMcThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("mcts_advance");
}

extern "C" int ka_mcts_advance(void* records, void* tree, int width, int simulations, int t, const void* table,
                               const int* model_of, int K, const float* pool_vlogits, const float* pool_rewards,
                               const void* pool_terminated, const void* pool_truncated, const void* step_err,
                               long long* actions, int* parent_row, int* active, int* pv, int* root_visits, float* root_values,
                               int* stats, int* err, int N, void* stream) {
    return ka_mcts_advance_explore(records, tree, width, simulations, t, table, model_of, K, pool_vlogits, pool_rewards,
                                   pool_terminated, pool_truncated, step_err, actions, parent_row, active, pv, root_visits,
                                   root_values, stats, err, nullptr, nullptr, nullptr, 0, nullptr, N, stream);
}
