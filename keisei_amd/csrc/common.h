// Shared device helpers for the keisei_amd HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

#define KA_OK 0
#define KA_ERR_ARG (-1)
#define KA_ERR_HIP (-2)
#define KA_ERR_UNSUPPORTED (-3)

#define KA_DTYPE_F32 0
#define KA_DTYPE_BF16 1

#define KA_BOARD 81       // 9x9 squares
#define KA_PADBOARD 121   // 11x11 zero-haloed board

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

struct bf16_t { uint16_t v; };   // storage type for bf16 tensors

// ---- error plumbing (host) -------------------------------------------------
void ka_set_error(const char* fmt, ...);
int ka_check_launch(const char* what);
#define KA_REQUIRE(cond, ...) do { if (!(cond)) { ka_set_error(__VA_ARGS__); return KA_ERR_ARG; } } while (0)
// every pointer of the list is a multiple of n bytes (NULL is)
inline bool ka_aligned(size_t n, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs) if ((uintptr_t)p % n != 0) return false;
    return true;
}

// Kernels that need more than 64 KiB of dynamic LDS: hipFuncAttributeMaxDynamicSharedMemorySize is a per-device
// property of the function, so it is set once per (kernel instantiation, device) -- `done` is that instantiation's
// bit mask of devices already configured (the only state the library keeps; written once per device, thread-safe).
#include <atomic>
inline int ka_big_lds_once(const void* func, std::atomic<unsigned long long>& done, const char* what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { ka_set_error("%s: hipGetDevice failed", what); return KA_ERR_HIP; }
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return KA_OK;
    if (hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
        ka_set_error("%s: hipFuncSetAttribute failed on device %d", what, dev);
        return KA_ERR_HIP;
    }
    done.fetch_or(bit, std::memory_order_release);
    return KA_OK;
}

// Ablation switches (KA_CONV_P_ABL, KA_CONV_T_ABL, KA_TOWER_ABL: they skip phases of a kernel and give WRONG results)
// exist only in diagnostic builds -- `KA_DIAG=1 python -m keisei_amd.build` compiles libkeisei_amd_diag.so with -DKA_DIAG;
// the product library never reads them.  (Switches that choose between two CORRECT implementations stay run-time; bench.py
// records every KA_* variable set in its environment.)
#include <stdlib.h>
inline const char* ka_diag_env(const char* name) {
#ifdef KA_DIAG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// ---- run-time switches (launch plan) ----------------------------------------------------------------------------------------
// Every KA_* switch the library honours is read from the environment ONCE -- at the first launch that asks, or again when
// the caller says so (ka_options_reload: tests and A/B tools that flip a switch inside one process) -- into a table the
// launchers index: no getenv() on the enqueue path.  bench.py records the switches set in its environment.
#define KA_OPTIONS(X)                                                                                                      \
    X(CONV_P) X(CONV_MT) X(CONV_PC2) X(CONV_PC2_SKIP) X(CONV_PC2_STAG) X(CONV_CORNER_IN) X(CONV_P_STAG) X(CONV_P_PRIO) X(CONV_P_WGS) X(CONV_P_NPW) X(CONV_WM) X(CONV_KC)       \
    X(CONV_NTW) X(CONV_STAGGER) X(CONV_PRIO) X(WGRAD_TN) X(WGRAD_WGS) X(WGRAD_STAG) X(WGRAD_LEAN) X(BOARD_PAIRS) X(TF_LDS_EPI) X(TF_K256) X(TF_BIG)    \
    X(TF_MAP2D) X(TF_ATTN_LDS) X(TF_ATTN_ONE) X(TAIL_FWD_KB) X(TAIL_GATE_P4)
enum KaOpt {
#define KA_OPT_ENUM(n) KA_OPT_##n,
    KA_OPTIONS(KA_OPT_ENUM)
#undef KA_OPT_ENUM
    KA_OPT_COUNT
};
struct KaOptVal { int set, val; };
const KaOptVal* ka_opts();                                   // capi.hip
inline bool ka_opt_set(KaOpt o) { return ka_opts()[o].set != 0; }
inline int ka_opt(KaOpt o, int dflt) { const KaOptVal v = ka_opts()[o]; return v.set ? v.val : dflt; }

// diagnostic only: [workgroup][8] stamp buffer of ka_debug_conv_stamps (slots 0 / 7: s_memtime at the start / end of the workgroup's
// main loop, 3 / 4: s_memrealtime there); null in production -- no stamp executes
std::atomic<unsigned long long*>& ka_debug_stamps();         // capi.hip

// Launch counts per dispatch form of the 3x3 convolutions and their weight gradient, read by ka_conv_route_counts: the tests see
// from these which kernel a (shape, batch, switch) combination reached.  Host-side, one relaxed increment per dispatch.
enum KaConvRoute {
    KA_RT_CONV,            // conv3x3_kernel (the generic form)
    KA_RT_PC,              // conv3x3_pc_kernel
    KA_RT_PC2,             // conv3x3_pc2_kernel, 128 channels (all 81 squares: no corner)
    KA_RT_PC2_CORNER_IN,   // conv3x3_pc2_kernel, 256 channels, square 80 as a sixth tile inside
    KA_RT_PC2_CORNER_OUT,  // conv3x3_pc2_kernel, 256 channels, square 80 left to the corner launch behind it
    KA_RT_CORNER,          // conv3x3_corner_kernel
    KA_RT_WGRAD_LEAN,      // wgrad_flat_kernel
    KA_RT_WGRAD_TILED,     // wgrad_kernel
    KA_RT_COUNT
};
void ka_conv_route(int r);                                   // conv3x3.hip

// ---- scalar conversions -----------------------------------------------------
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
// Plain cast: hipcc emits v_cvt_pk_bf16_f32 (RNE, NaN stays NaN) on gfx950.
__device__ __forceinline__ uint16_t f2bf(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int kSize = 4;
    static constexpr int kPer16 = 4;      // elements per 16-byte piece
    static constexpr int kDtype = KA_DTYPE_F32;
    typedef f32x4 vec16;
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
    static __device__ __forceinline__ void unpack(const vec16& v, float* f) {
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    }
    static __device__ __forceinline__ vec16 pack(const float* f) { vec16 v = {f[0], f[1], f[2], f[3]}; return v; }
};
template <> struct Elem<bf16_t> {
    static constexpr int kSize = 2;
    static constexpr int kPer16 = 8;
    static constexpr int kDtype = KA_DTYPE_BF16;
    typedef bf16x8 vec16;
    static __device__ __forceinline__ float ld(const bf16_t* p) { return bf2f(p->v); }
    static __device__ __forceinline__ void st(bf16_t* p, float v) { p->v = f2bf(v); }
    static __device__ __forceinline__ void unpack(const vec16& v, float* f) {
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
    }
    static __device__ __forceinline__ vec16 pack(const float* f) {
        vec16 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (__bf16)f[i];
        return v;
    }
};

// pair (2-element) access used by the board kernels: one thread owns 2 adjacent channels
template <typename T> __device__ __forceinline__ f32x2 ld2(const T* p);
template <> __device__ __forceinline__ f32x2 ld2<float>(const float* p) { return *reinterpret_cast<const f32x2*>(p); }
template <> __device__ __forceinline__ f32x2 ld2<bf16_t>(const bf16_t* p) {
    uint32_t u = *reinterpret_cast<const uint32_t*>(p);
    f32x2 r = {__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
    return r;
}
template <typename T> __device__ __forceinline__ void st2(T* p, f32x2 v);
template <> __device__ __forceinline__ void st2<float>(float* p, f32x2 v) { *reinterpret_cast<f32x2*>(p) = v; }
template <> __device__ __forceinline__ void st2<bf16_t>(bf16_t* p, f32x2 v) {
    uint32_t u = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    *reinterpret_cast<uint32_t*>(p) = u;
}
// round-trip through the storage type (so statistics see exactly what is stored)
template <typename T> __device__ __forceinline__ float rnd(float v);
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<bf16_t>(float v) { return bf2f(f2bf(v)); }

// padded-board index of square p (0..80) on the 11x11 haloed grid
__device__ __forceinline__ int pad_index(int p) { return (p / 9 + 1) * 11 + (p % 9) + 1; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// Integer sum / max over a workgroup of THREADS threads (whole waves); red: THREADS / 64 ints of LDS.  Every thread calls
// it and every thread gets the result.  The leading barrier lets the same `red` serve one reduction after another.
template <int THREADS> __device__ __forceinline__ int ka_block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
    for (int w = 0; w < THREADS / 64; ++w) r += red[w];
    return r;
}
template <int THREADS> __device__ __forceinline__ int ka_block_max(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = red[0];
    for (int w = 1; w < THREADS / 64; ++w) r = max(r, red[w]);
    return r;
}
// The same over floats.  The order of the additions is part of the result: the wave's butterfly, then wave 0's partial plus
// those of waves 1, 2, ... in turn.  Every kernel that reduces a policy row (loss.hip, sampling.hip, insight.hip,
// lookahead.hip) sums through this body, which is why their normalisers agree to the bit.
template <int THREADS> __device__ __forceinline__ float ka_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < THREADS / 64; ++w) r += red[w];
    return r;
}
template <int THREADS> __device__ __forceinline__ float ka_block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < THREADS / 64; ++w) r = fmaxf(r, red[w]);
    return r;
}

// One fp32 row copied by a workgroup of THREADS threads: 8-byte vectors where the row length and both addresses allow it
// (a 50 x 9 x 9 observation row is 16 200 B: 8-byte aligned, not 16).
template <int THREADS> __device__ __forceinline__ void ka_copy_row(float* dst, const float* src, int n, int tid) {
    if ((n & 1) == 0 && (((uintptr_t)dst | (uintptr_t)src) & 7) == 0) {
        const f32x2* s2 = reinterpret_cast<const f32x2*>(src);
        f32x2* d2 = reinterpret_cast<f32x2*>(dst);
        for (int i = tid; i < n / 2; i += THREADS) d2[i] = s2[i];
    } else {
        for (int i = tid; i < n; i += THREADS) dst[i] = src[i];
    }
}

// The splitmix64 finaliser behind every draw on the device (the samplers' uniforms, the league's opponents and sides, the
// SL mirror, the env's position hash): ONE body, so the same (seed, key) gives the same bits in every kernel and in the
// numpy restatement (league_rollout._mix).  kKaWeyl is also the step by which a ply advances the sampler seed.
constexpr unsigned long long kKaWeyl = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ unsigned long long ka_mix64(unsigned long long x) {
    x += kKaWeyl;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains the vector-memory counter, i.e. it waits
// for every global load in flight (a weight prefetch issued before the barrier) and for global stores to complete
#define KA_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// The rollout's scalar value (katago_ppo.py:536-541 / value_adapter.py:56-65): P(W) - P(L) of the three value logits at
// vl, blended with clamp(score_lead, -1, 1) by alpha when there is a score.  ONE body for ka_policy_sample and
// ka_policy_sample_play (loss.hip's policy_sample_kernel), ka_scalar_value and the plan kernels of ka_league_step and
// ka_selfplay_step, which hand it to rollout_rows.h's write_row: the rows of a rollout and the sampler's values agree bit
// for bit.
__device__ __forceinline__ float ka_blended_value(const float* vl, const float* score, float alpha) {
    const float l0 = vl[0], l1 = vl[1], l2 = vl[2];
    const float m = fmaxf(l0, fmaxf(l1, l2));
    const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
    float v = (e0 - e2) / (e0 + e1 + e2);
    if (score && alpha != 0.f) v = (1.f - alpha) * v + alpha * fminf(fmaxf(*score, -1.f), 1.f);
    return v;
}

// Inclusive prefix sum of v over the 64 lanes of a wave, in lane order.
__device__ __forceinline__ int ka_wave_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// Ranks of the flagged threads of one 256-thread tile, in thread order, behind the `running` flagged threads of the tiles
// before it: *rank = running + (flagged threads below this one), -1 for a thread that is not flagged.  Returns the tile's
// count.  One ballot per wave and a sum over the four waves (wsum: 4 ints of LDS): no atomics, so the order is the thread
// order.  Every thread of the workgroup calls it.  Shared by the arena's record_pre / features_step, the league's and the
// self-play step's plan kernels and the game log's step.
__device__ __forceinline__ int ka_tile_rank(bool want, int running, int* wsum, int* rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(want);
    __syncthreads();                                           // the tile before has read wsum
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int off = running, tot = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) off += wsum[w];
        tot += wsum[w];
    }
    *rank = want ? off + __popcll(b & ((1ull << lane) - 1ull)) : -1;
    return tot;
}
