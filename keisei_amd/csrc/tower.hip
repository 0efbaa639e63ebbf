// Eval-mode residual tower in ONE launch (rollout inference, katago_ppo.py:543-617 ->
// se_resnet.py:67-75 x num_blocks under torch.no_grad() in eval mode).
//
// In eval mode no tensor couples the boards: BatchNorm uses its running statistics (a per-channel affine), the global-pool
// bias and the squeeze-excite gate are per-board reductions.  So one 512-thread workgroup carries ONE board through all
// the blocks: the board (81 x 256 bf16) and the intermediate h live in LDS, the two 3x3 convolutions of a block are the
// same implicit GEMM as conv3x3.hip (zero-haloed 17-wide LDS image of a 128-channel chunk, 9 taps as constant LDS
// offsets, fragment-ordered weights streamed L2 -> registers four k-steps ahead, out^T accumulators so a lane owns 8
// consecutive channels of a square), and everything between them stays in registers / LDS:
//   g    = W2 relu(W1 [mean|max|std](x) + b1) + b2               (global-pool bias, a per-board matrix-vector chain)
//   h    = relu(bn1(conv1(x))) + g                                 (conv1 epilogue -> LDS)
//   z    = bn2(conv2(h))                                           (accumulators)
//   s    = V2 relu(V1 mean_p(z) + c1) + c2                         (squeeze-excite chain)
//   x'   = relu(z * sigmoid(s[:C]) + s[C:] + x)                    (-> LDS, in place) and its pooled mean / max / std
// Replaces, per call of select_actions at 128 environments, 80 conv + 80 FC-chain + 40 tail launches (4.6 ms of GPU time)
// by one launch.  bf16 activations, C = 256.
//
// Grouped forms (league / tournament play: many models of one shape, each on a few boards of one batch): the same kernel
// with a per-board model index, model_of[b] -> row m of a (K, nblocks, 14) pointer table, at C = 128 or 256, plus a grouped
// stem (input conv 50 -> C, input_bn, ReLU, pooled statistics: the conv is the tower's own MFMA loop over one 128-channel
// chunk) and grouped heads.  A board whose index lies outside [0, K) is unseated: it reads no weights, its outputs are zeros.
// At C = 128 a block has 8 output tiles: waves 0..3 own two tiles each (the 8-consecutive-channel accumulator layout of
// C = 256 unchanged), waves 4..7 only join the image builds and the FC chains.
#include <stdlib.h>
#include "common.h"

namespace {

constexpr int kKC = 128;
constexpr int kPW = 17;                                   // squares per padded board row (as conv3x3.hip)
constexpr int kImgSquares = 10 * kPW + 11;                // 181
constexpr int kImgStride = kKC * 2 + 32;                  // 288 B: conflict-free 16-lane fragment reads
constexpr int kZeroSquares = 2 * (kPW + 1) + 1;           // all-zero squares behind the image: what the padded rows (81 -> 96) read

template <int kC> struct TowerLayout {                    // LDS layout of a C-channel board
    static constexpr int kNatStride = kC * 2;             // natural [81][C] bf16
    static constexpr int kXn = 0, kHn = kXn + KA_BOARD * kNatStride, kImg = kHn + KA_BOARD * kNatStride;
    static constexpr int kVec = kImg + (kImgSquares + kZeroSquares) * kImgStride;     // float vectors
    static constexpr int kPooled = 0, kGbias = 3 * kC, kHid = kGbias + kC, kSeMean = kHid + 256, kSeHid = kSeMean + kC,
                         kSeOut = kSeHid + 64;
    static constexpr int kVecFloats = kSeOut + 2 * kC;
    static constexpr int kLds = kVec + kVecFloats * 4;
};

enum TowerMode { kTowerOne = 0, kTowerGrouped = 1, kStemGrouped = 2 };

struct TowerBlock {              // device table row, 14 pointers (int64 each on the host side)
    const char* w1; const char* w2;                       // fragment-ordered conv weights (ka_pack_conv3x3, mode 0)
    const float *sc1, *sh1, *sc2, *sh2;                   // eval-mode BatchNorm scale / shift
    const float *gw1, *gb1, *gw2, *gb2;                   // global_fc: (G, 3C), (G), (C, G), (C)
    const float *sw1, *sb1, *sw2, *sb2;                   // se_fc1 (R, C), (R); se_fc2 (2C, R), (2C)
};
struct StemRow {                 // device table row of the grouped stem, 3 pointers
    const char* w;                                        // input_conv packed with Ci zero-padded to 128 (ka_pack_conv3x3 mode 0)
    const float *sc, *sh;                                 // input_bn eval scale / shift
};
struct TowerArgs {
    const uint16_t* x_in; const float* pool_in; uint16_t* x_out; float* pool_out;
    const TowerBlock* blocks; int nblocks, B, G, R;
    int abl;                     // diagnostics only (KA_TOWER_ABL): 1 skip the global-pool chain, 2 skip the SE chain, 4 skip the image builds, 8 skip the MFMA steps
    const int* model_of; int K;  // grouped forms: model of board b; blocks is then (K, nblocks) rows
    const float* obs; const StemRow* stems; int cin;      // grouped stem: obs (B, cin, 9, 9) fp32
};

// pointers read from the device table are generic to the compiler: loads through them would be FLAT loads, which count on
// the LDS counter as well -- every wait for an LDS fragment would then also wait for the weight prefetch.  Cast to global.
typedef const __attribute__((address_space(1))) bf16x8* gfrag_ptr;
typedef const __attribute__((address_space(1))) float* gfloat_ptr;
__device__ __forceinline__ gfloat_ptr gf(const float* p) { return (gfloat_ptr)(p); }

__device__ __forceinline__ int img_square(int p) { return (p / 9 + 1) * kPW + (p % 9) + 1; }
__device__ __forceinline__ float row16_sum(float v) {     // over the 16 lanes that share q (lane bits 0..3)
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 4)); v = fmaxf(v, __shfl_xor(v, 8));
    return v;
}
__device__ __forceinline__ float row16_min(float v) {
    v = fminf(v, __shfl_xor(v, 1)); v = fminf(v, __shfl_xor(v, 2)); v = fminf(v, __shfl_xor(v, 4)); v = fminf(v, __shfl_xor(v, 8));
    return v;
}

template <int kC, int kMode>
__global__ __launch_bounds__(512) void tower_eval_kernel(TowerArgs a) {
    typedef TowerLayout<kC> L;
    constexpr int kNatStride = L::kNatStride, kXn = L::kXn, kHn = L::kHn, kImg = L::kImg, kVec = L::kVec;
    constexpr int kPooled = L::kPooled, kGbias = L::kGbias, kHid = L::kHid, kSeMean = L::kSeMean, kSeHid = L::kSeHid,
                  kSeOut = L::kSeOut;
    constexpr int kNT = kC / 16;                          // output tiles of a convolution
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* vec = reinterpret_cast<float*>(smem + kVec);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.x;
    const int c0 = wave * 32 + q * 8;                     // this lane's 8 output channels
    const bool active = kC == 256 || wave < kC / 32;      // the waves that own output channels (all 8 at C = 256)
    const TowerBlock* blocks = a.blocks;
    StemRow stem{};
    if constexpr (kMode != kTowerOne) {
        const int m = __builtin_amdgcn_readfirstlane(a.model_of[b]);
        if (m < 0 || m >= a.K) {                          // unseated board: reads no weights, writes zeros
            for (int i = tid; i < KA_BOARD * kC / 8; i += 512)
                reinterpret_cast<uint4*>(a.x_out + (size_t)b * KA_BOARD * kC)[i] = uint4{0, 0, 0, 0};
            for (int i = tid; i < 4 * kC; i += 512) a.pool_out[(size_t)b * 4 * kC + i] = 0.f;
            return;
        }
        if constexpr (kMode == kTowerGrouped) blocks += (size_t)m * a.nblocks;
        else stem = a.stems[m];
    }
    // ---- board and its pooled statistics into LDS; the image halo is zeroed once
    for (int i = tid; i < (kImgSquares + kZeroSquares) * kImgStride / 16; i += 512) reinterpret_cast<uint4*>(smem + kImg)[i] = uint4{0, 0, 0, 0};
    if constexpr (kMode == kStemGrouped) {
        // obs planes as bf16 (what ka_obs_to_nhwc stores) into channels 0..127 of the natural layout, zero past cin
        const float* ob = a.obs + (size_t)b * a.cin * KA_BOARD;
        for (int i = tid; i < kKC * KA_BOARD; i += 512) {
            const int c = i / KA_BOARD, p = i - c * KA_BOARD;
            *reinterpret_cast<__bf16*>(smem + kXn + p * kNatStride + c * 2) = (__bf16)(c < a.cin ? ob[i] : 0.f);
        }
    } else {
        for (int i = tid; i < KA_BOARD * kC / 8; i += 512)
            reinterpret_cast<uint4*>(smem + kXn)[i] = reinterpret_cast<const uint4*>(a.x_in + (size_t)b * KA_BOARD * kC)[i];
        for (int i = tid; i < 3 * kC; i += 512) vec[kPooled + i] = a.pool_in[(size_t)b * 4 * kC + i];
    }

    // activation-fragment row offsets of this lane (6 row tiles; rows >= 81 are never stored)
    int rowoff[6];
#pragma unroll
    for (int mt = 0; mt < 6; ++mt) {
        const int p = mt * 16 + r;
        // (padded rows read zeros: zero operands cost the matrix pipe less power, and the clock is what the power budget leaves)
        rowoff[mt] = kImg + (p < KA_BOARD ? img_square(p) : kImgSquares + kPW + 1) * kImgStride + q * 16;
    }
    f32x4 acc[6][2];

    // one 3x3 convolution: src = natural-layout input in LDS, w = fragment-ordered weights with ksg k-steps of 32 input
    // channels per tap (C / 32 in the tower, 4 for the stem's 128-channel padded input), nk 128-channel chunks of src
    auto conv = [&](int src, const char* w, int nk, int ksg) {
#pragma unroll
        for (int mt = 0; mt < 6; ++mt) { acc[mt][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        const char* wl = w + (size_t)(wave * 2) * 1024 + lane * 16;       // + ((tap*ksg + ks)*kNT) * 1024 per k-step, + 1024 for the 2nd tile
        auto wfrag = [&](int kc, int step, bf16x8 (&f)[2]) {              // step = tap*4 + ks4 within the chunk (clamped)
            step = min(step, 35);
            const int tap = step >> 2, ks = kc * 4 + (step & 3);
            const char* p = wl + (size_t)((tap * ksg + ks) * kNT) * 1024;
            f[0] = *(gfrag_ptr)(p);
            f[1] = *(gfrag_ptr)(p + 1024);
        };
        for (int kc = 0; kc < nk; ++kc) {
            bf16x8 w0[2], w1[2], w2[2], w3[2];
            if (active) { wfrag(kc, 0, w0); wfrag(kc, 1, w1); wfrag(kc, 2, w2); }   // in flight across the image build
            KA_LDS_BARRIER();                                              // the image's previous readers are done; src is complete
            if (!(a.abl & 4)) for (int i = tid; i < KA_BOARD * 16; i += 512) {
                const int row = i >> 4, pc = i & 15;
                *reinterpret_cast<uint4*>(smem + kImg + img_square(row) * kImgStride + pc * 16) =
                    *reinterpret_cast<const uint4*>(smem + src + row * kNatStride + kc * 256 + pc * 16);
            }
            KA_LDS_BARRIER();
            if (!active) continue;
            auto toff_of = [&](int step) {
                step = min(step, 35);
                const int tap = step >> 2, ks = step & 3;
                return ((tap / 3 - 1) * kPW + (tap % 3 - 1)) * kImgStride + ks * 64;
            };
            // activation fragments are double-buffered across k-steps: the 6 LDS reads of step s + 1 are issued one in
            // front of every pair of MFMAs of step s (issue order pinned), so an MFMA never waits for the read just issued
            auto mm = [&](const bf16x8 (&wf)[2], const bf16x8 (&ac)[6], bf16x8 (&an)[6], int next_step) {
                const int toff = toff_of(next_step);
#pragma unroll
                for (int mt = 0; mt < 6; ++mt) {
                    an[mt] = *reinterpret_cast<const bf16x8*>(smem + rowoff[mt] + toff);
                    acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0], ac[mt], acc[mt][0], 0, 0, 0);
                    acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1], ac[mt], acc[mt][1], 0, 0, 0);
                }
#pragma unroll
                for (int mt = 0; mt < 6; ++mt) {
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                }
            };
            bf16x8 fa[6], fb[6];
            {
                const int toff = toff_of(0);
#pragma unroll
                for (int mt = 0; mt < 6; ++mt) fa[mt] = *reinterpret_cast<const bf16x8*>(smem + rowoff[mt] + toff);
            }
#pragma unroll 1
            for (int tap = 0; tap < ((a.abl & 8) ? 0 : 9); ++tap) {      // weights of step s + 3 are requested before step s multiplies
                const int s0 = tap * 4;
                wfrag(kc, s0 + 3, w3); __builtin_amdgcn_sched_barrier(0); mm(w0, fa, fb, s0 + 1); __builtin_amdgcn_sched_barrier(0);
                wfrag(kc, s0 + 4, w0); __builtin_amdgcn_sched_barrier(0); mm(w1, fb, fa, s0 + 2); __builtin_amdgcn_sched_barrier(0);
                wfrag(kc, s0 + 5, w1); __builtin_amdgcn_sched_barrier(0); mm(w2, fa, fb, s0 + 3); __builtin_amdgcn_sched_barrier(0);
                wfrag(kc, s0 + 6, w2); __builtin_amdgcn_sched_barrier(0); mm(w3, fb, fa, s0 + 4); __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // pooled mean / max / std of the board v (bf16-rounded values; rows >= 81 ignored) into vec[kPooled..]
    auto pool_stats = [&](const float (&v)[6][8]) {
        float sum[8], mx[8], mn[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { sum[e] = 0.f; mx[e] = -INFINITY; mn[e] = INFINITY; }
#pragma unroll
        for (int mt = 0; mt < 6; ++mt) {
            if (mt * 16 + r < KA_BOARD) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { sum[e] += v[mt][e]; mx[e] = fmaxf(mx[e], v[mt][e]); mn[e] = fminf(mn[e], v[mt][e]); }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float mean = row16_sum(sum[e]) * (1.f / KA_BOARD);
            const float hi = row16_max(mx[e]), lo = row16_min(mn[e]);
            float m2 = 0.f;
#pragma unroll
            for (int mt = 0; mt < 6; ++mt) { const float d = v[mt][e] - mean; m2 += (mt * 16 + r < KA_BOARD) ? d * d : 0.f; }
            m2 = row16_sum(m2);
            if (r == 0) {
                vec[kPooled + c0 + e] = mean;
                vec[kPooled + kC + c0 + e] = hi;
                vec[kPooled + 2 * kC + c0 + e] = hi == lo ? 0.f : sqrtf(m2 * (1.f / KA_BOARD));   // a constant plane: exactly 0
            }
        }
    };

    KA_LDS_BARRIER();
    if constexpr (kMode == kStemGrouped) {
        // ---- stem: x = relu(input_bn(input_conv(obs))) and its pooled statistics (the per-layer path's conv + tail launches)
        conv(kXn, stem.w, 1, kKC / 32);
        if (active) {
            float sc[8], sh[8], v[6][8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { sc[e] = gf(stem.sc)[c0 + e]; sh[e] = gf(stem.sh)[c0 + e]; }
#pragma unroll
            for (int mt = 0; mt < 6; ++mt) {
                const int p = mt * 16 + r;
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // the conv output is rounded to bf16 first, as the stand-alone conv stores it
                    const float y = (float)(__bf16)(e < 4 ? acc[mt][0][e] : acc[mt][1][e - 4]);
                    o[e] = (__bf16)fmaxf(fmaf(y, sc[e], sh[e]), 0.f);
                    v[mt][e] = (float)o[e];
                }
                if (p < KA_BOARD) *reinterpret_cast<bf16x8*>(smem + kXn + p * kNatStride + c0 * 2) = o;
            }
            pool_stats(v);
        }
        KA_LDS_BARRIER();
    }
    // Every workgroup walks the same FC weight rows, and all of them arrive at a chain at about the same moment: without a
    // per-workgroup rotation of the row order all 128+ workgroups ask the same L2 lines in the same clock (one channel serves
    // them one after the other while the others idle).  The rows are independent, so the order does not touch the results.
    const int rot1 = (int)((blockIdx.x * 8u) % (unsigned)a.G), rot2 = (int)((blockIdx.x * 16u) & (kC - 1));
    for (int blk = 0; blk < (kMode == kStemGrouped ? 0 : a.nblocks); ++blk) {
        const TowerBlock tb = blocks[blk];
        // ---- global-pool bias: hid = relu(W1 pooled + b1), one wave per row, lanes along the 3C inputs; four rows' loads are
        // in flight together (a dependent chain of L2 round trips per row is what this phase would otherwise be)
        if (!(a.abl & 1)) {
            // 16-byte loads, eight rows (24 loads per lane) in flight together: the phase is a chain of L2 round trips
            typedef const __attribute__((address_space(1))) f32x4* gvec_ptr;
            constexpr int kPv = (3 * kC / 4 + 63) / 64;         // 16-byte pieces of the pooled vector per lane (3 at C = 256)
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
            f32x4 pv[kPv];
#pragma unroll
            for (int k = 0; k < kPv; ++k) pv[k] = lane + 64 * k < 3 * kC / 4 ? *reinterpret_cast<const f32x4*>(vec + kPooled + 4 * (lane + 64 * k)) : z4;
            for (int jb = wave; jb < a.G; jb += 64) {
                f32x4 wv[8][kPv];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = (min(jb + 8 * u, a.G - 1) + rot1) % a.G;          // (rows rotated per workgroup, see rot1)
                    gvec_ptr wr = (gvec_ptr)(tb.gw1 + (size_t)j * 3 * kC);
#pragma unroll
                    for (int k = 0; k < kPv; ++k) wv[u][k] = lane + 64 * k < 3 * kC / 4 ? wr[lane + 64 * k] : z4;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float t = 0.f;
#pragma unroll
                    for (int k = 0; k < kPv; ++k) t += wv[u][k][0] * pv[k][0] + wv[u][k][1] * pv[k][1] + wv[u][k][2] * pv[k][2] + wv[u][k][3] * pv[k][3];
                    t = wave_sum(t);
                    const int j = jb + 8 * u, jr = (j + rot1) % a.G;
                    if (lane == 0 && j < a.G) vec[kHid + jr] = fmaxf(t + gf(tb.gb1)[jr], 0.f);
                }
            }
        }
        KA_LDS_BARRIER();
        if (!(a.abl & 1) && (kC == 256 || tid < 2 * kC)) {   // g[c] = W2[c] . hid + b2[c]: two threads per channel, each a contiguous half of the row (16-byte loads)
            typedef const __attribute__((address_space(1))) f32x4* gvec_ptr;
            const int c = ((tid >> 1) + rot2) & (kC - 1), half = tid & 1, n = a.G >> 1;
            gvec_ptr wr = (gvec_ptr)(tb.gw2 + (size_t)c * a.G + half * n);
            float s = 0.f;
            for (int j = 0; j < n / 4; ++j) {
                const f32x4 w4 = wr[j];
                const float* hv = vec + kHid + half * n + 4 * j;
                s += w4[0] * hv[0] + w4[1] * hv[1] + w4[2] * hv[2] + w4[3] * hv[3];
            }
            s += __shfl_xor(s, 1);
            if (half == 0) vec[kGbias + c] = s + gf(tb.gb2)[c];
        }
        // ---- conv1 and its epilogue: h = relu(bn1(y1)) + g   (the first barrier inside conv publishes g)
        conv(kXn, tb.w1, kC / kKC, kC / 32);
        if (active) {
            float sc[8], sh[8], gb[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { sc[e] = gf(tb.sc1)[c0 + e]; sh[e] = gf(tb.sh1)[c0 + e]; gb[e] = vec[kGbias + c0 + e]; }
#pragma unroll
            for (int mt = 0; mt < 6; ++mt) {
                const int p = mt * 16 + r;
                if (p < KA_BOARD) {
                    bf16x8 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // y1 is rounded to bf16 first, as the stand-alone kernels store it, then transformed and rounded again
                        const float y0 = (float)(__bf16)acc[mt][0][e], y1 = (float)(__bf16)acc[mt][1][e];
                        o[e] = (__bf16)(fmaxf(fmaf(y0, sc[e], sh[e]), 0.f) + gb[e]);
                        o[4 + e] = (__bf16)(fmaxf(fmaf(y1, sc[4 + e], sh[4 + e]), 0.f) + gb[4 + e]);
                    }
                    *reinterpret_cast<bf16x8*>(smem + kHn + p * kNatStride + c0 * 2) = o;
                }
            }
        }
        // ---- conv2; z = bn2(y2) stays in the accumulators
        conv(kHn, tb.w2, kC / kKC, kC / 32);
        if (active) {
            float sc[8], sh[8], sm[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { sc[e] = gf(tb.sc2)[c0 + e]; sh[e] = gf(tb.sh2)[c0 + e]; sm[e] = 0.f; }
#pragma unroll
            for (int mt = 0; mt < 6; ++mt) {
                const bool ok = mt * 16 + r < KA_BOARD;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // (the squeeze is the mean of the fp32 conv output, as the conv epilogue of the stand-alone path takes it)
                    sm[e] += ok ? acc[mt][0][e] : 0.f; sm[4 + e] += ok ? acc[mt][1][e] : 0.f;
                    acc[mt][0][e] = fmaf((float)(__bf16)acc[mt][0][e], sc[e], sh[e]);
                    acc[mt][1][e] = fmaf((float)(__bf16)acc[mt][1][e], sc[4 + e], sh[4 + e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = row16_sum(sm[e]);
                if (r == 0) vec[kSeMean + c0 + e] = fmaf(t * (1.f / KA_BOARD), sc[e], sh[e]);   // mean_p bn2(y2)
            }
        }
        KA_LDS_BARRIER();
        if (!(a.abl & 2)) {   // se hidden: one wave per row, the loads of all this wave's rows in flight together
            float mv[kC / 64];
#pragma unroll
            for (int k = 0; k < kC / 64; ++k) mv[k] = vec[kSeMean + lane + 64 * k];
            for (int jb = wave; jb < a.R; jb += 32) {
                float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = min(jb + 8 * u, a.R - 1);
                    gfloat_ptr wr = gf(tb.sw1) + (size_t)j * kC;
#pragma unroll
                    for (int k = 0; k < kC / 64; ++k) s[u] += wr[lane + 64 * k] * mv[k];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = jb + 8 * u;
                    const float t = wave_sum(s[u]);
                    if (lane == 0 && j < a.R) vec[kSeHid + j] = fmaxf(t + gf(tb.sb1)[j], 0.f);
                }
            }
        }
        KA_LDS_BARRIER();
        if (!(a.abl & 2) && (kC == 256 || tid < 2 * kC)) {
            gfloat_ptr wr = gf(tb.sw2) + (size_t)tid * a.R;   // thread k < 2C = 512: gate logits | shifts
            float s = gf(tb.sb2)[tid];
            if ((a.R & 3) == 0) {
                typedef const __attribute__((address_space(1))) f32x4* gvec_ptr;
                gvec_ptr w4p = (gvec_ptr)(tb.sw2 + (size_t)tid * a.R);
                for (int j = 0; j < a.R / 4; ++j) {
                    const f32x4 w4 = w4p[j];
                    const float* hv = vec + kSeHid + 4 * j;
                    s += w4[0] * hv[0] + w4[1] * hv[1] + w4[2] * hv[2] + w4[3] * hv[3];
                }
            } else {
                for (int j = 0; j < a.R; ++j) s += wr[j] * vec[kSeHid + j];
            }
            vec[kSeOut + tid] = tid < kC ? sigmoidf_(s) : s;
        }
        KA_LDS_BARRIER();
        // ---- x' = relu(z * gate + shift + x) in place, and its pooled statistics (a wave owns all squares of its channels)
        if (active) {
            float gate[8], shf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { gate[e] = vec[kSeOut + c0 + e]; shf[e] = vec[kSeOut + kC + c0 + e]; }
            float v[6][8];
#pragma unroll
            for (int mt = 0; mt < 6; ++mt) {
                const int p = mt * 16 + r;
                const bool ok = p < KA_BOARD;
                bf16x8 xr = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ok) xr = *reinterpret_cast<const bf16x8*>(smem + kXn + p * kNatStride + c0 * 2);
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float z = e < 4 ? acc[mt][0][e] : acc[mt][1][e - 4];
                    o[e] = (__bf16)fmaxf(fmaf(z, gate[e], shf[e]) + (float)xr[e], 0.f);
                    v[mt][e] = (float)o[e];
                }
                if (ok) *reinterpret_cast<bf16x8*>(smem + kXn + p * kNatStride + c0 * 2) = o;
            }
            pool_stats(v);
        }
        KA_LDS_BARRIER();
    }
    for (int i = tid; i < KA_BOARD * kC / 8; i += 512)
        reinterpret_cast<uint4*>(a.x_out + (size_t)b * KA_BOARD * kC)[i] = reinterpret_cast<const uint4*>(smem + kXn)[i];
    for (int i = tid; i < 4 * kC; i += 512) a.pool_out[(size_t)b * 4 * kC + i] = i < 3 * kC ? vec[kPooled + i] : 0.f;
}

// ---- grouped heads: one 256-thread workgroup per board, everything from the board's LDS copy.  policy_conv1 (1x1, C -> P),
// policy_bn1 (eval affine), ReLU, policy_conv2 (1x1, P -> 139, bias); value / score: FC chains over the pooled [mean|max|std].
struct HeadRow {                 // device table row of the grouped heads, 13 pointers
    const float *wp1, *scp, *shp;                         // policy_conv1 (P, C); policy_bn1 eval scale / shift (P)
    const float *wp2, *bp2;                               // policy_conv2 (139, P), (139)
    const float *v1w, *v1b, *v2w, *v2b;                   // value_fc1 (V, 3C), (V); value_fc2 (3, V), (3)
    const float *s1w, *s1b, *s2w, *s2b;                   // score_fc1 (S, 3C), (S); score_fc2 (1, S), (1)
};
struct HeadArgs {
    const uint16_t* x; const float* pool; const int* model_of; const HeadRow* heads; int K, P, V, S;
    float *logits, *value, *score;
};
constexpr int kHeadThreads = 256, kMoves = 139;

__host__ __device__ constexpr size_t heads_lds(int C, int P, int V, int S) {   // x [81][C] bf16 | p1 [81][P] | pooled [3C] | hv [V] | hs [S]
    return (size_t)KA_BOARD * C * 2 + ((size_t)KA_BOARD * P + 3 * C + V + S) * 4;
}

template <int kC>
__global__ __launch_bounds__(kHeadThreads) void heads_grouped_kernel(HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int P = a.P, V = a.V, S = a.S;
    float* p1 = reinterpret_cast<float*>(smem + KA_BOARD * kC * 2);
    float* pooled = p1 + KA_BOARD * P;
    float* hv = pooled + 3 * kC;
    float* hs = hv + V;
    float* lg = a.logits + (size_t)b * KA_BOARD * kMoves;
    const int m = __builtin_amdgcn_readfirstlane(a.model_of[b]);
    if (m < 0 || m >= a.K) {                              // unseated board: zeros
        for (int i = tid; i < KA_BOARD * kMoves; i += kHeadThreads) lg[i] = 0.f;
        if (tid < 3) a.value[(size_t)b * 3 + tid] = 0.f;
        if (tid == 0) a.score[b] = 0.f;
        return;
    }
    const HeadRow h = a.heads[m];
    for (int i = tid; i < KA_BOARD * kC / 8; i += kHeadThreads)
        reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(a.x + (size_t)b * KA_BOARD * kC)[i];
    for (int i = tid; i < 3 * kC; i += kHeadThreads) pooled[i] = a.pool[(size_t)b * 4 * kC + i];
    __syncthreads();
    // p1[p][j] = relu(bn(sum_c x[p][c] W1[j][c]))
    for (int i = tid; i < KA_BOARD * P; i += kHeadThreads) {
        const int p = i / P, j = i - p * P;
        const bf16x8* xr = reinterpret_cast<const bf16x8*>(smem + p * kC * 2);
        const f32x4* wr = reinterpret_cast<const f32x4*>(h.wp1 + (size_t)j * kC);
        float s = 0.f;
#pragma unroll 4
        for (int k = 0; k < kC / 8; ++k) {
            const bf16x8 xv = xr[k];
            const f32x4 w0 = wr[2 * k], w1 = wr[2 * k + 1];
            s += (float)xv[0] * w0[0] + (float)xv[1] * w0[1] + (float)xv[2] * w0[2] + (float)xv[3] * w0[3]
               + (float)xv[4] * w1[0] + (float)xv[5] * w1[1] + (float)xv[6] * w1[2] + (float)xv[7] * w1[3];
        }
        p1[i] = fmaxf(fmaf(s, h.scp[j], h.shp[j]), 0.f);
    }
    // value / score hidden layers: one wave per row, lanes along the 3C pooled inputs
    for (int j = wave; j < V + S; j += kHeadThreads / 64) {
        const float* wr = j < V ? h.v1w + (size_t)j * 3 * kC : h.s1w + (size_t)(j - V) * 3 * kC;
        float t = 0.f;
        for (int k = lane; k < 3 * kC; k += 64) t += wr[k] * pooled[k];
        t = wave_sum(t);
        if (lane == 0) {
            if (j < V) hv[j] = fmaxf(t + h.v1b[j], 0.f);
            else hs[j - V] = fmaxf(t + h.s1b[j - V], 0.f);
        }
    }
    __syncthreads();
    // logits[p][o] = b2[o] + sum_j p1[p][j] W2[o][j]   ((B, 9, 9, 139) layout: o fastest)
    for (int i = tid; i < KA_BOARD * kMoves; i += kHeadThreads) {
        const int p = i / kMoves, o = i - p * kMoves;
        const float* wr = h.wp2 + (size_t)o * P;
        const float* pr = p1 + p * P;
        float s = h.bp2[o];
        for (int j = 0; j < P; ++j) s += pr[j] * wr[j];
        lg[i] = s;
    }
    // value (waves 0..2, one output each) and score (wave 3)
    {
        const int n = wave < 3 ? V : S;
        const float* wr = wave < 3 ? h.v2w + (size_t)wave * V : h.s2w;
        const float* hid = wave < 3 ? hv : hs;
        float t = 0.f;
        for (int j = lane; j < n; j += 64) t += wr[j] * hid[j];
        t = wave_sum(t);
        if (lane == 0) {
            if (wave < 3) a.value[(size_t)b * 3 + wave] = t + h.v2b[wave];
            else a.score[b] = t + h.s2b[0];
        }
    }
}

}  // namespace

// 1 when the one-launch tower covers this configuration (bf16 activations, 256 channels, FC widths it holds in LDS)
extern "C" int ka_tower_eval_supported(int C, int G, int R, int dtype) {
    return dtype == KA_DTYPE_BF16 && C == 256 && G >= 8 && G <= 256 && G % 8 == 0 && R >= 1 && R <= 64;
}

// x_out, pool_out = the residual tower applied to x_in (B, 81, C) bf16 with pooled statistics pool_in (B, 4C); blocks =
// device table of nblocks x 14 pointers (TowerBlock).  Eval mode only (BatchNorm as scale/shift).
extern "C" int ka_tower_eval(const void* x_in, const float* pool_in, void* x_out, float* pool_out, const void* blocks,
                             int nblocks, int B, int C, int G, int R, int dtype, void* stream) {
    KA_REQUIRE(x_in && pool_in && x_out && pool_out && blocks && nblocks > 0 && B > 0, "tower_eval: bad arguments");
    KA_REQUIRE(ka_tower_eval_supported(C, G, R, dtype), "tower_eval: unsupported configuration C=%d G=%d R=%d dtype=%d", C, G, R, dtype);
    TowerArgs a{static_cast<const uint16_t*>(x_in), pool_in, static_cast<uint16_t*>(x_out), pool_out,
                static_cast<const TowerBlock*>(blocks), nblocks, B, G, R, 0, nullptr, 0, nullptr, nullptr, 0};
    if (const char* e = ka_diag_env("KA_TOWER_ABL")) a.abl = atoi(e);
    static std::atomic<unsigned long long> done{0};
    if (int rc = ka_big_lds_once(reinterpret_cast<const void*>(&tower_eval_kernel<256, kTowerOne>), done, "tower_eval")) return rc;
    hipLaunchKernelGGL((tower_eval_kernel<256, kTowerOne>), dim3(B), dim3(512), TowerLayout<256>::kLds,
                       static_cast<hipStream_t>(stream), a);
    return ka_check_launch("tower_eval");
}

// ---- grouped forms (one launch each, whatever the number of models) -------------------------------------------------------
extern "C" int ka_tower_eval_grouped_supported(int C, int G, int R, int dtype) {
    return dtype == KA_DTYPE_BF16 && (C == 128 || C == 256) && G >= 8 && G <= 256 && G % 8 == 0 && R >= 1 && R <= 64;
}

template <int kMode>
static int tower_grouped_launch(const TowerArgs& a, int C, hipStream_t st, const char* what) {
    static std::atomic<unsigned long long> done128{0}, done256{0};
    if (C == 128) {
        if (int rc = ka_big_lds_once(reinterpret_cast<const void*>(&tower_eval_kernel<128, kMode>), done128, what)) return rc;
        hipLaunchKernelGGL((tower_eval_kernel<128, kMode>), dim3(a.B), dim3(512), TowerLayout<128>::kLds, st, a);
    } else {
        if (int rc = ka_big_lds_once(reinterpret_cast<const void*>(&tower_eval_kernel<256, kMode>), done256, what)) return rc;
        hipLaunchKernelGGL((tower_eval_kernel<256, kMode>), dim3(a.B), dim3(512), TowerLayout<256>::kLds, st, a);
    }
    return ka_check_launch(what);
}

// x_out (B, 81, C) bf16, pool_out (B, 4C) = relu(input_bn(input_conv(obs))) of board b with the stem of model model_of[b];
// stems = device table of K rows of 3 pointers (StemRow: input_conv packed by ka_pack_conv3x3 mode 0 with Ci padded to 128,
// input_bn eval scale, shift).  obs (B, cin, 9, 9) fp32, cin <= 128.
extern "C" int ka_stem_eval_grouped(const float* obs, const int* model_of, const void* stems, int K, void* x_out,
                                    float* pool_out, int B, int cin, int C, int dtype, void* stream) {
    KA_REQUIRE(obs && model_of && stems && x_out && pool_out && K > 0 && B > 0, "stem_eval_grouped: bad arguments");
    KA_REQUIRE(cin >= 1 && cin <= kKC, "stem_eval_grouped: %d input planes (at most %d)", cin, kKC);
    KA_REQUIRE(dtype == KA_DTYPE_BF16 && (C == 128 || C == 256), "stem_eval_grouped: unsupported C=%d dtype=%d", C, dtype);
    TowerArgs a{nullptr, nullptr, static_cast<uint16_t*>(x_out), pool_out, nullptr, 0, B, 0, 0, 0,
                model_of, K, obs, static_cast<const StemRow*>(stems), cin};
    return tower_grouped_launch<kStemGrouped>(a, C, static_cast<hipStream_t>(stream), "stem_eval_grouped");
}

// ka_tower_eval with a model per board: tables = device table (K, nblocks, 14) pointers (TowerBlock rows), board b runs
// the blocks of model model_of[b]; a board with model_of[b] outside [0, K) reads no weights and gets zeros.
extern "C" int ka_tower_eval_grouped(const void* x_in, const float* pool_in, void* x_out, float* pool_out, const int* model_of,
                                     const void* tables, int K, int nblocks, int B, int C, int G, int R, int dtype, void* stream) {
    KA_REQUIRE(x_in && pool_in && x_out && pool_out && model_of && tables && K > 0 && nblocks > 0 && B > 0,
               "tower_eval_grouped: bad arguments");
    KA_REQUIRE(ka_tower_eval_grouped_supported(C, G, R, dtype), "tower_eval_grouped: unsupported configuration C=%d G=%d R=%d dtype=%d",
               C, G, R, dtype);
    TowerArgs a{static_cast<const uint16_t*>(x_in), pool_in, static_cast<uint16_t*>(x_out), pool_out,
                static_cast<const TowerBlock*>(tables), nblocks, B, G, R, 0, model_of, K, nullptr, nullptr, 0};
    return tower_grouped_launch<kTowerGrouped>(a, C, static_cast<hipStream_t>(stream), "tower_eval_grouped");
}

// policy logits (B, 9, 9, 139), value logits (B, 3), score (B, 1), all fp32, of board b with the heads of model model_of[b]
// (zeros for an unseated board); x (B, 81, C) bf16 and pool (B, 4C) are the tower's outputs; heads = device table of K rows
// of 13 pointers (HeadRow).  P <= 32, V, S <= 512.
extern "C" int ka_heads_eval_grouped(const void* x, const float* pool, const int* model_of, const void* heads, int K,
                                     float* logits, float* value, float* score, int B, int C, int P, int V, int S, int dtype,
                                     void* stream) {
    KA_REQUIRE(x && pool && model_of && heads && logits && value && score && K > 0 && B > 0, "heads_eval_grouped: bad arguments");
    KA_REQUIRE(dtype == KA_DTYPE_BF16 && (C == 128 || C == 256) && P >= 1 && P <= 32 && V >= 1 && V <= 512 && S >= 1 && S <= 512,
               "heads_eval_grouped: unsupported configuration C=%d P=%d V=%d S=%d dtype=%d", C, P, V, S, dtype);
    HeadArgs a{static_cast<const uint16_t*>(x), pool, model_of, static_cast<const HeadRow*>(heads), K, P, V, S, logits, value, score};
    const size_t lds = heads_lds(C, P, V, S);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (C == 128) hipLaunchKernelGGL(heads_grouped_kernel<128>, dim3(B), dim3(kHeadThreads), lds, st, a);
    else hipLaunchKernelGGL(heads_grouped_kernel<256>, dim3(B), dim3(kHeadThreads), lds, st, a);
    return ka_check_launch("heads_eval_grouped");
}
