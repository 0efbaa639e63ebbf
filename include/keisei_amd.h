/* keisei_amd.h -- C ABI of libkeisei_amd.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * Keisei KataGo-PPO training hot path.
 *
 * The reference (tachyon-beep/keisei) has NO native boundary on this path: every operator below is a
 * PyTorch op call site inside keisei/training/{models/se_resnet,katago_ppo,gae,value_adapter}.py
 * (SURVEY.md 2.3 K1-K23).  This header therefore defines the boundary a binding would add *underneath*
 * the reference's Python API; each entry point cites the reference statement(s) it replaces
 * (paths relative to the reference repository root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise;
 *     the library never allocates, frees or retains memory -- workspaces are caller-provided;
 *   - every launch goes to `stream` (a hipStream_t passed as void*); nothing synchronises;
 *   - return value: 0 = launched, <0 = error (KA_ERR_*), message via ka_last_error() (thread-local);
 *   - `dtype`: activation storage type of (B,81,C) NHWC tensors, KA_DTYPE_F32 (exact-fp32 MFMA / FMA,
 *     parity mode) or KA_DTYPE_BF16 (bf16 MFMA with fp32 accumulate, throughput mode);
 *   - "board" = one 9x9 position = 81 squares; activations are NHWC: element (b, p, c) at
 *     ((b*81 + p)*C + c); per-channel / per-board vectors are fp32.
 */
#ifndef KEISEI_AMD_H
#define KEISEI_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define KA_OK 0
#define KA_ERR_ARG (-1)
#define KA_ERR_HIP (-2)
#define KA_ERR_UNSUPPORTED (-3)
#define KA_DTYPE_F32 0
#define KA_DTYPE_BF16 1

/* ---- library identity / errors ------------------------------------------------------------ */
int ka_version(void);
const char* ka_target_arch(void);          /* "gfx950" */
const char* ka_last_error(void);           /* message of the last failing call on this thread */
/* Run-time switches (KA_CONV_*, KA_WGRAD_*, KA_TF_*, ...; csrc/common.h KA_OPTIONS) are read from the environment ONCE, by the
 * first launch that asks, into the table the launchers index (no getenv() on the enqueue path).  A process that changes one
 * afterwards calls ka_options_reload() (returns the number of switches set). */
int ka_options_reload(void);

/* ---- 3x3 convolution (implicit GEMM on MFMA) ----------------------------------------------------
 * Replaces nn.Conv2d(Cin, Cout, 3, padding=1, bias=False): input_conv / conv1 / conv2
 * (models/se_resnet.py:50,52,110,140) and, with a mode-1 weight pack, autograd's data gradient.
 * Optional fused input transform x' = relu?(x*in_scale[c] + in_shift[c]) + in_bias[b,c] reproduces
 * `F.relu(self.bn1(...)) + g.unsqueeze(-1).unsqueeze(-1)` (se_resnet.py:71,78) on the fly.
 * Epilogue outputs (optional): bsum[b,n] = sum over the 81 squares of the fp32 result (SE squeeze,
 * se_resnet.py:83, and the BatchNorm mean), sqpart[r,n] = per-board sum of squares
 * (r < ka_conv3x3_sqpart_rows(B)).  Requires Cin % 32 == 0 (bf16) / 16 (f32), Cout % 16 == 0. */
int ka_conv3x3_fwd(const void* in, const void* wpack, void* out, const float* in_scale, const float* in_shift,
                   const float* in_bias, int relu, float* bsum, float* sqpart, int B, int Cin, int Cout, int dtype,
                   void* stream);
/* ka_conv3x3_fwd that also writes the transformed input x' (the tensor `F.relu(self.bn1(...)) + g...` of se_resnet.py:71,78, which the
 * reference materialises and autograd saves for conv2's weight gradient) to x_out (B, 81, Cin), so that ka_conv3x3_wgrad reads it as
 * a plain operand instead of repeating the transform per tile.  x_out == NULL: ka_conv3x3_fwd.  Shapes: ka_conv3x3_fwd_keep_supported. */
int ka_conv3x3_fwd_keep_supported(int B, int Cin, int Cout, int dtype);
int ka_conv3x3_fwd_keep(const void* in, const void* wpack, void* out, const float* in_scale, const float* in_shift,
                        const float* in_bias, int relu, float* bsum, float* sqpart, void* x_out, int B, int Cin, int Cout, int dtype,
                        void* stream);
int ka_conv3x3_sqpart_rows(int B);
/* launch counts per dispatch form of ka_conv3x3_* and ka_conv3x3_wgrad into a host array of n counts, in this order: generic
   kernel, producer / consumer kernel, two-board kernel at 128 channels, two-board kernel at 256 channels with square 80 inside,
   two-board kernel at 256 channels with the corner launch behind it, corner launch, lean weight gradient, tiled weight
   gradient.  Host-side counters: tests check that a case reached the route it claims to cover. */
int ka_conv_route_counts(long long* out, int n);
/* Data-gradient convolution with the surrounding BatchNorm-backward passes fused in (bf16): the input is
 * dy = in*k[0:C] + k[C:2C] + in2*k[2C:3C] (= ka_bn_bwd_apply on the fly, also written to dy_out for the weight-gradient
 * kernel); with ep_y the output is masked by the ReLU of the preceding BatchNorm, out = conv(dy)*[ep_scale*ep_y+ep_shift>0],
 * and ep_s1/ep_s2 [ka_conv3x3_sqpart_rows(B)][Cout] receive the partial sums of ka_relu_bn_bwd_reduce.  bsum = per-board
 * sums of the unmasked conv(dy) (gradient of the global-pool bias, se_resnet.py:78). */
int ka_conv3x3_dgrad_fused(const void* in, const void* in2, const float* k, void* dy_out, const void* wpack, void* out,
                           float* bsum, const void* ep_y, const float* ep_scale, const float* ep_shift,
                           const float* ep_mean, const float* ep_invstd, float* ep_s1, float* ep_s2, int B, int Cin,
                           int Cout, int dtype, void* stream);
/* ka_conv3x3_dgrad_fused with the gradient input in factored form: `du` and gate_add = [gate | add] ([2][B][Cin] fp32) with
 * dz = du * gate[b,c] + add[b,c] -- the gradient wrt bn2's output, se_resnet.py:86-90 backward: the ReLU-masked gradient of the
 * block output times the SE gate plus the squeeze path's per-board term -- as ka_block_dx_tail_bwd_du_gate leaves it.  dz is
 * formed in fp32 inside the input transform (never rounded to bf16, never stored): dy = dz*k[0:C] + k[C:2C] + in2*k[2C:3C].
 * Shapes: ka_conv3x3_dgrad_gated_supported (the two-board tower kernel: B >= 512, 256 or 128 channels, bf16). */
int ka_conv3x3_dgrad_gated_supported(int B, int Cin, int Cout, int dtype, int masked);
int ka_conv3x3_dgrad_fused_gated(const void* du, const float* gate_add, const void* in2, const float* k,
                                 void* dy_out, const void* wpack, void* out, float* bsum, const void* ep_y,
                                 const float* ep_scale, const float* ep_shift, const float* ep_mean, const float* ep_invstd,
                                 float* ep_s1, float* ep_s2, int B, int Cin, int Cout, int dtype, void* stream);
/* (Co,Ci,3,3) fp32 torch-layout weights -> MFMA B-fragment order (a derived cache; the stored parameter keeps
 * the reference's shape).  mode 0: forward, Nout = Co, Kin = Ci rounded up (zero channels); mode 1: data
 * gradient (in/out swapped, taps flipped), Nout = Ci, Kin = Co.  dst bytes = 9*(Kin/cpk)*(Nout/16)*1024. */
int ka_pack_conv3x3(const float* w, void* dst, int Co, int Ci, int Nout, int Kin, int mode, int dtype, void* stream);
/* Every layer of a network in one launch.  table = device int64 [n][8]: {src weights, dst pack, Co, Ci, Nout, Kin,
 * mode, 0} per entry, as the arguments of ka_pack_conv3x3; max_pieces = max over entries of 9*(Kin/cpk)*(Nout/16)*64. */
int ka_pack_conv3x3_multi(const long long* table, int n, long long max_pieces, int dtype, void* stream);
/* Weight gradient dW[n,c,ky,kx] = sum_{b,p} dY[b,p,n] * X'[b,p+tap,c] (autograd conv2d weight backward);
 * X' uses the same fused input transform as the forward.  slab: ka_wgrad_splits(B,Cin,Cout,target_wgs)*9*Cout*Cin floats. */
int ka_conv3x3_wgrad(const void* dy, const void* x, const float* in_scale, const float* in_shift, const float* in_bias,
                     int relu, float* slab, float* dw, int B, int Cin, int Cin_real, int Cout, int accumulate,
                     int target_wgs, int dtype, void* stream);
int ka_wgrad_splits(int B, int Cin, int Cout, int target_wgs);   /* target_wgs: 0 = 256 (one workgroup per CU) */
int ka_debug_conv_stamps(unsigned long long* stamps);   /* diagnostics only (tools/conv_stamps.py); null = off */

/* ---- layout at the model boundary ----------------------------------------------------------------
 * obs (S,Cobs,9,9) fp32 NCHW -> (B,81,Cpad) NHWC; row b is obs[idx[b]] when idx != NULL, which fuses the
 * minibatch gather `gpu_obs[idx]` (katago_ppo.py:835) into the first kernel. */
int ka_obs_to_nhwc(const float* obs, const long long* idx, void* out, int B, int Cobs, int Cpad, int dtype, void* stream);
int ka_nhwc_to_nchw(const void* in, float* out, int B, int C, int dtype, void* stream);

/* ---- BatchNorm2d, training and eval (se_resnet.py:51,53,111,121; torch defaults eps 1e-5, momentum 0.1) --
 * ka_bn_reduce: sums[0:C] = sum_b bsum[b,c], sums[C:2C] = sum_r sqpart[r,c] in fp64, fixed order
 *   (part: workspace of ka_reduce_workspace_doubles(C) doubles).  Between reduce and coeffs a caller may
 *   all-reduce `sums` across ranks (SyncBatchNorm, katago_loop.py:495-496) and pass the global element count
 *   through count_dev (device double) instead of `count`.
 * ka_bn_coeffs: scale = gamma*invstd, shift = beta - mean*scale; updates running_mean / running_var (unbiased)
 *   / num_batches_tracked exactly like nn.BatchNorm2d when the pointers are non-NULL. */
int ka_reduce_workspace_doubles(int C);
int ka_bn_reduce(const float* bsum, int B, const float* sqpart, int R, int C, double* sums, double* part, void* stream);
int ka_bn_coeffs(const double* sums, double count, const double* count_dev, const float* gamma, const float* beta,
                 float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                 float* scale, float* shift, float* mean, float* invstd, int C, void* stream);
int ka_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, float* scale, float* shift, int C, void* stream);
/* the same for n layers in one launch (eval-mode nn.BatchNorm2d at se_resnet.py:51,53,111,121): device table of n rows {gamma, beta, running_mean, running_var, scale, shift,
 * C, eps as float bits} (8 x int64 each); max_c = largest C.  Rollout inference: 82 launches -> 1. */
int ka_bn_eval_coeffs_multi(const long long* table, int n, int max_c, void* stream);
/* backward: sums = [sum dz | sum dz*yhat]; dgamma/dbeta from the LOCAL sums, dy = k[0:C]*dz + k[C:2C] + k[2C:3C]*y
 * from the (all-reduced) global sums; train = 0 gives the eval-mode derivative. */
int ka_pair_reduce(const float* p1, const float* p2, int B, int C, double* sums, double* part, void* stream);
int ka_bn_bwd_coeffs(const double* sums_local, const double* sums_global, double count, const double* count_dev,
                     const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta, float* k,
                     int C, int train, void* stream);
/* SyncBatchNorm (katago_loop.py:495-496; torch's SyncBatchNorm all_gathers (mean, invstd, count) forward and all_reduces
 * (sum_dy, sum_dy_xmu) backward): sums[0:2C] as above from the two row sets, sums[2C] = count -- ONE vector for the caller's
 * single all-reduce per layer and direction; local_copy (optional, [2C+1]) keeps the un-reduced values (dgamma / dbeta). */
int ka_sync_reduce(const float* p1, int rows1, const float* p2, int rows2, int C, double count, double* sums,
                   double* local_copy, double* part, void* stream);
/* One launch less per BatchNorm layer when no cross-rank reduction sits between the two steps: ka_bn_reduce /
 * ka_pair_reduce with sums == NULL stop after their first stage, and these read the partials in `part` directly. */
int ka_bn_coeffs_parts(const double* part, double count, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, long long* num_batches_tracked, float momentum, float eps, float* scale,
                       float* shift, float* mean, float* invstd, int C, void* stream);
int ka_bn_bwd_coeffs_parts(const double* part, double count, const float* gamma, const float* mean, const float* invstd,
                           float* dgamma, float* dbeta, float* k, int C, int train, void* stream);
/* ... and the two steps as ONE launch (nn.BatchNorm2d's training statistics, se_resnet.py:51,53, and their autograd backward):
 * ka_bn_reduce(sums = NULL) + ka_bn_coeffs_parts, ka_pair_reduce(sums = NULL) + ka_bn_bwd_coeffs_parts.  The workgroup that
 * finishes a 64-channel column group last computes the group's coefficients from the 64 partial rows in slice order (same values
 * as the two launches, bit for bit).  counters: (C + 63) / 64 ints, zero before the first use and left zero; one such launch at
 * a time per (part, counters) pair. */
int ka_bn_reduce_coeffs(const float* bsum, int B, const float* sqpart, int R, int C, double* part, int* counters, double count,
                        const float* gamma, const float* beta, float* running_mean, float* running_var,
                        long long* num_batches_tracked, float momentum, float eps, float* scale, float* shift, float* mean,
                        float* invstd, void* stream);
int ka_pair_reduce_bwd_coeffs(const float* p1, const float* p2, int rows, int C, double* part, int* counters, double count,
                              const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta, float* k,
                              int train, void* stream);
int ka_bn_bwd_apply(const void* dz, const void* y, const float* k, void* dy, int B, int C, int dtype, void* stream);
int ka_affine_rows(const float* in, const float* a, const float* s, float mul, float* out, int B, int C, void* stream);

/* ---- GlobalPoolBiasBlock tail and global pooling (se_resnet.py:74-77,83-98) ----------------------------
 * out = relu((scale*y+shift) * sigmoid(se[b,c]) + se[b,C+c] + res); pool[b] = [mean | max | std(correction=0) |
 * number of squares attaining the max] of `out` (4C floats; the 4th plane serves amax's tie-splitting backward).
 * se == NULL and res == NULL give relu(bn(y)) (stem, se_resnet.py:140). */
int ka_block_tail_fwd(const void* y, const float* scale, const float* shift, const float* se, const void* res, void* out,
                      float* pool, int B, int C, int dtype, void* stream);
/* ka_block_tail_fwd with the squeeze-excite FC chain of the block inside (se_resnet.py:83-86: se = se_fc2(relu(se_fc1(mean over the
 * squares of bn2(y))))): z = scale * (bsum / 81) + shift from the conv's per-board sums, h = relu(W1 z + b1), se = W2 h + b2, then the
 * tail as above with that se.  sqz_out (B,C) / se1_out (B,H) / se_out (B,2C) receive z, h and se for the backward -- the tensors
 * ka_fc_chain leaves when the chain is a launch of its own in front of ka_block_tail_fwd.  Shapes: ka_block_tail_fwd_se_supported. */
int ka_block_tail_fwd_se_supported(int C, int H, int dtype);
int ka_block_tail_fwd_se(const void* y, const float* scale, const float* shift, const float* bsum, const float* W1, const float* b1,
                         const float* W2, const float* b2, const void* res, void* out, float* pool, float* sqz_out, float* se1_out,
                         float* se_out, int B, int C, int H, int dtype, void* stream);
int ka_pool_fwd(const void* x, float* pool, int B, int C, int dtype, void* stream);
/* backward of the tail: dse = [sigmoid'(a)*sum_p du*z | sum_p du] with du = dout*[out>0]; then
 * dz = du*sigmoid(a) + dsq/81 plus the per-board BatchNorm partial sums s1p = sum dz, s2p = sum dz*yhat. */
int ka_tail_bwd_reduce(const void* dout, const void* out, const void* y, const float* scale, const float* shift,
                       const float* se, float* dse, int B, int C, int dtype, void* stream);
int ka_tail_bwd_dz(const void* dout, const void* out, const void* y, const float* se, const float* dsq, const float* mean,
                   const float* invstd, void* dz, float* s1p, float* s2p, int B, int C, int dtype, void* stream);
/* Single-pass form of the two calls above plus the squeeze-excite FC chain backward that sits between them
 * (se_resnet.py:77-86: se_fc2 -> ReLU -> se_fc1): dse (B,2C) and dh = masked gradient of the hidden layer (B,H) are
 * written for the FC weight-gradient GEMMs, dz / s1p / s2p as ka_tail_bwd_dz.  W2 = se_fc2.weight (2C,H),
 * W1 = se_fc1.weight (H,C), se1 = the saved hidden activations (B,H).  ka_tail_bwd_fused_supported() says whether
 * the shape fits the register-resident board tile. */
int ka_tail_bwd_fused_supported(int C, int H, int dtype);
int ka_tail_bwd_fused(const void* dout, const void* out, const void* y, const float* scale, const float* shift,
                      const float* se, const float* se1, const float* W2, const float* W1, const float* mean,
                      const float* invstd, void* dz, float* dse, float* dh, float* s1p, float* s2p, int B, int C, int H,
                      int dtype, void* stream);
/* da = dh*[scale*y+shift > 0] (ReLU after BatchNorm) + the same partial sums */
int ka_relu_bn_bwd_reduce(const void* dh, const void* y, const float* scale, const float* shift, const float* mean,
                          const float* invstd, void* da, float* s1p, float* s2p, int B, int C, int dtype, void* stream);
/* dx = [dxc] + [dout*[out>0]] + backward of [mean|max|std] pooling of x (ties of amax share the gradient, std
 * gradient is 0 where sigma == 0), using xpool = ka_block_tail_fwd's pool of x; dpool is (B,3C). */
int ka_block_dx(const void* dxc, const void* dout, const void* out, const void* x, const float* xpool, const float* dpool,
                void* dx, int B, int C, int dtype, void* stream);
/* The two calls that meet at a block boundary of the backward pass in ONE launch: ka_block_dx of the block above (its
 * result dx is this block's output gradient, its x this block's output: se_resnet.py:89-90, residual + ReLU) followed by
 * ka_tail_bwd_fused of this block -- x, dxc, dout_up, out_up, y are read once and dx, dz written (7 activation passes instead
 * of 9).  dx is rounded to the activation dtype before it is used: every output equals the two-launch sequence bit for bit.
 * dxc may be NULL; dout_up and out_up are both NULL where the gradient enters the tower from the heads (se_resnet.py:147-157). */
int ka_block_dx_tail_bwd_supported(int C, int H, int dtype);
/* The kernel form the board launches take for a shape; launches nothing (the tests assert the form they ran).  kernel 0:
 * ka_block_tail_fwd / ka_pool_fwd, 1: ka_block_dx, 2: ka_tail_bwd_fused, 3: ka_block_dx_tail_bwd[_du], 4: ..._du_gate (H is read
 * by 2..4).  0 = not covered; else threads + 1024 * squares per thread + 65536 * flags (1: 16-byte pieces -- clear: channel
 * pairs, passes in bits 20.. --, 2: FC weights pre-loaded, 4: loads batched when dxc and du_up are given, 8: half-width pieces). */
int ka_board_form(int kernel, int C, int H, int dtype);
int ka_block_dx_tail_bwd(const void* dxc, const void* dout_up, const void* out_up, const void* x, const float* xpool,
                         const float* dpool, void* dx, const void* y, const float* scale, const float* shift, const float* se,
                         const float* se1, const float* W2, const float* W1, const float* mean, const float* invstd, void* dz,
                         float* dse, float* dh, float* s1p, float* s2p, int B, int C, int H, int dtype, void* stream);
/* The same launch as a CHAIN over the block boundaries, one activation read shorter.  All that the residual branch one block
 * further down takes from dx is du = dx * [x > 0] (se_resnet.py:90: the ReLU after the residual sum) -- the value this launch
 * forms for its own tail -- so du_out = dx * [x > 0] is written instead of dx, and du_up (the du_out of the launch above; NULL
 * where the gradient enters from the heads) is added as it is: the block above's output is not read (4 activation reads + 2
 * writes).  dz / dse / dh / s1p / s2p equal ka_block_dx_tail_bwd's bit for bit; ka_block_dx takes a du_out as its `dout`
 * unchanged (masking twice by the same output changes nothing), which ends the chain at the first block. */
int ka_block_dx_tail_bwd_du(const void* dxc, const void* du_up, const void* x, const float* xpool, const float* dpool,
                            void* du_out, const void* y, const float* scale, const float* shift, const float* se,
                            const float* se1, const float* W2, const float* W1, const float* mean, const float* invstd, void* dz,
                            float* dse, float* dh, float* s1p, float* s2p, int B, int C, int H, int dtype, void* stream);
/* The chain launch WITHOUT dz (4 activation reads + 1 write): dz = du_out * gate_out[b,c] + add_out[b,c] (gate = sigmoid of the
 * SE gate logits, add = dsq / 81: se_resnet.py:83-90 backward) has a single reader, the conv2 data gradient, which takes the three
 * through ka_conv3x3_dgrad_fused_gated.  bf16(fmaf(du_out, gate_out, add_out)) is ka_block_dx_tail_bwd_du's dz bit for bit;
 * du_out / dse / dh / s1p / s2p are the same bits. */
int ka_block_dx_tail_bwd_du_gate(const void* dxc, const void* du_up, const void* x, const float* xpool, const float* dpool,
                                 void* du_out, const void* y, const float* scale, const float* shift, const float* se,
                                 const float* se1, const float* W2, const float* W1, const float* mean, const float* invstd,
                                 float* gate_out, float* add_out, float* dse, float* dh, float* s1p, float* s2p, int B, int C,
                                 int H, int dtype, void* stream);

/* ---- small dense layers: nn.Linear / 1x1 nn.Conv2d forward and backward (se_resnet.py:57-61,65-66,120-130) --
 * C[M,N] (+)= act(opA(A)[M,K] * opB(B)[K,N] + bias); opA(A)[m,k] = transA ? A[k*lda+m] : A[m*lda+k], likewise opB.
 * *_bf16 flags mark bf16 operands/outputs; nsplit > 1 writes raw fp32 partial slabs (reduce with ka_reduce_slabs). */
int ka_gemm(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int lda, int ldb, int ldc,
            int transA, int transB, int a_bf16, int b_bf16, int c_bf16, int relu, int accumulate, int nsplit, void* stream);
/* waves per workgroup (4 or 16) of the kernel ka_gemm launches for this output shape and split count: a pure query */
int ka_gemm_waves(int M, int N, int nsplit);
/* Every FC weight / bias gradient of a backward pass in one launch (autograd's nn.Linear weight / bias backward for
 * se_resnet.py:57-66 global_fc / se_fc1 / se_fc2 and :125-130 value / score heads): job j computes dW_j (N,K) = dY_j^T X_j and, when db_j
 * is non-zero, db_j (N) = column sums of dY_j (dY_j (M,N) fp32; X_j M rows of ldx floats or bf16).  table: device int64
 * [njobs][10] = {dY, X, dW, db, M, N, K, ldx, x_bf16, first workgroup of the job}; a job owns ceil(N/64) *
 * ceil((K + (db != 0)) / 64) consecutive workgroups, total_wgs = their sum.  No split-K: one fixed summation order. */
int ka_gemm_grouped_wgrad(const long long* table, int njobs, int total_wgs, void* stream);
/* Two chained FC layers in one launch (se_resnet.py:57-66 global_fc / se_fc1+se_fc2, :125-130 value / score heads):
 *   y (M,N2) = W2 (N2,H) * relu(W1 (H,K1) * x' + b1) + b2,   x' = x (M rows of ldx floats, first K1 used), or with
 *   in_scale/in_shift: x'[m,k] = in_scale[k] * (x[m,k] * in_alpha) + in_shift[k] (the SE squeeze from the conv's per-board
 *   sums).  x_out (M,K1) / hidden_out (M,H) optionally keep x' / the ReLU'd hidden rows for the backward.  Exact f32
 *   matrix instructions, fp32 accumulation.  ka_fc_chain_supported() tells whether a shape is handled (K1 % 16, H in
 *   {16,32,64} or a multiple of 16 >= 128, ...); otherwise issue ka_gemm twice. */
int ka_fc_chain_supported(int K1, int ldx, int H, int N2);
int ka_fc_chain(const float* x, const float* in_scale, const float* in_shift, float in_alpha, const float* W1,
                const float* b1, const float* W2, const float* b2, float* x_out, float* hidden_out, float* y, int M, int K1,
                int ldx, int H, int N2, void* stream);
/* backward of such a chain with respect to its input, one launch: dhidden = (dy W2) * [hidden > 0] (written: the dY of W1's
 * weight gradient), dx = dhidden W1; W2T (H, N2) and W1T (K1, H) are transposed copies of the nn.Linear weights kept current
 * by ka_transpose_multi (table rows {src, dst, rows, cols}).  Replaces autograd's input gradients of global_fc
 * (se_resnet.py:62-63, 71). */
int ka_fc_chain_bwd(const float* dy, const float* hidden, const float* W2T, const float* W1T, float* dhidden_out, float* dx,
                    int M, int N2, int H, int K1, void* stream);
int ka_transpose_multi(const void* table, int n, int max_tiles, void* stream);
int ka_reduce_slabs(const float* slab, float* out, int nsplit, long long n, int accumulate, void* stream);
/* two slab sets of one split count in one launch (a layer's weight- and bias-gradient partials); same sums, same order */
int ka_reduce_slabs2(const float* slab_a, float* out_a, long long na, const float* slab_b, float* out_b, long long nb, int nsplit,
                     void* stream);
int ka_colsum(const float* A, const float* Bm, float* part, float* part2, int M, int N, int nsplit, void* stream);
int ka_relu_mask(float* g, const float* h, long long n, void* stream);
/* policy-head BatchNorm over fp32 rows (M = B*81, N = policy_channels; se_resnet.py:121,144) */
int ka_rows_affine_relu(const float* in, const float* scale, const float* shift, float* out, long long M, int N, void* stream);
int ka_rows_sq_sums(const float* A, float* part, float* part2, int M, int N, int nsplit, void* stream);
int ka_rows_bn_sums(const float* da, const float* in, const float* mean, const float* invstd, float* part, float* part2,
                    int M, int N, int nsplit, void* stream);
int ka_rows_bn_bwd(float* dr, const float* in, const float* p0, const float* p1, long long M, int N, int mode, void* stream);

/* ---- fused KataGo-PPO minibatch loss (katago_ppo.py:857-924, :33-57; value_adapter.py:98-126) -----------
 * ka_policy_loss: masked log-softmax over A = 11259 actions, log-prob gather, clipped surrogate, entropy over
 *   legal actions -- per-sample terms AND dL/dlogits in one pass over the logits.  Per-sample inputs (legal,
 *   actions, old_lp, adv) are rows of the epoch dataset addressed through idx (NULL = identity).
 *   w_policy = lambda_policy/B, w_entropy = entropy_coeff/B; gscale = optional device loss scale (GradScaler).
 *   flags[0] |= NaN in raw logits, flags[1] |= 1: a sample without legal action (the reference's two guards,
 *   katago_ppo.py:861-871), flags[1] |= 2: an action id outside [0, A) (the reference's gather traps on the device).
 *   legal: bool rows (S,A) when legal_words == 0, else packed rows (S,legal_words) uint32 with bit j of word w = action
 *   32 w + j and legal_words == ka_mask_words(A) -- the device rollout store's column (ka_rollout_append).
 * ka_value_loss: W/D/L cross-entropy (ignore_index -1, all-ignored -> 0), score MSE, their gradients, the mean
 *   reductions of the per-sample policy terms, and the value metrics of compute_value_metrics (katago_ppo.py:60-78).
 *   out[9] = {policy_loss, value_ce, score_mse, entropy, total, n_valid, value_accuracy, frac_win, frac_draw};
 *   acc[4] += {policy, value (combined lambda-weighted when combined_value_metric), score, entropy}. */
int ka_policy_loss(const float* logits, const void* legal, const long long* actions, const float* old_lp, const float* adv,
                   const long long* idx, float* dlogits, float* new_lp, float* rowloss, float* rowent, int* flags,
                   const float* gscale, float clip_eps, float w_policy, float w_entropy, int B, int A, int legal_words,
                   void* stream);
/* Rollout action selection (katago_ppo.py:566-584): probs[b] = softmax of logits[b] over the legal actions, 0 elsewhere;
 * nlegal[b] = number of legal actions (0 -> the caller raises the reference's error); flags[0] |= NaN in the logits.
 * legal as in ka_policy_loss (bool rows, or packed rows with legal_words = ka_mask_words(A)). */
int ka_masked_softmax(const float* logits, const void* legal, float* probs, int* nlegal, int* flags, int B, int A,
                      int legal_words, void* stream);
/* ka_policy_sample: the whole tail of select_actions in one launch (katago_ppo.py:567-612 masked_fill / softmax /
 * Categorical.sample / log_prob / zero-legal guard, :536-541 scalar value, value_adapter.py:56-65 blend).  logits (B,A) fp32 or
 * bf16 (logits_bf16 != 0); legal as in ka_masked_softmax; seed: any 64-bit value, one uniform per (seed, row) by a 64-bit mix;
 * actions (B) int64, logp (B) = log softmax_masked(logits)[action], nlegal (B); values (B) optional: P(W)-P(L) of vlogits (B,3),
 * blended with clamp(score,-1,1) by alpha when score != NULL.  flags[0] |= NaN in the logits, flags[1] |= a row with no legal action. */
int ka_policy_sample(const void* logits, int logits_bf16, const void* legal, int legal_words, long long seed,
                     const float* vlogits, const float* score, float alpha, long long* actions, float* logp, float* values,
                     int* nlegal, int* flags, int B, int A, void* stream);
/* ka_policy_sample_play: ka_policy_sample for league play (no value output).  The seed is read from *seed_dev (device int64),
 * so a captured graph draws fresh randomness on every replay; a row with model_of[b] outside [0, K) gets its first legal
 * action (the lowest set bit of its mask row) and log-prob 0.  Seated rows: same actions and log-probs as ka_policy_sample
 * with the same seed value; nlegal and flags as there. */
int ka_policy_sample_play(const void* logits, int logits_bf16, const void* legal, int legal_words, const long long* seed_dev,
                          const int* model_of, int K, long long* actions, float* logp, int* nlegal, int* flags, int B, int A,
                          void* stream);
/* Supervised policy cross-entropy (keisei/sl/trainer.py:150-152): rowloss[b] = logsumexp(logits[b]) - logits[b][t],
 * t = targets[idx ? idx[b] : b]; dlogits (optional) = w_policy * (softmax - onehot) [* *gscale].  flags[0] |= NaN logits,
 * flags[1] |= target outside [0,A).  ka_value_loss then supplies the W/D/L cross-entropy, the score MSE and the means
 * (rowent = zeros, entropy_coeff = 0). */
int ka_policy_ce(const float* logits, const long long* targets, const long long* idx, float* dlogits, float* rowloss,
                 int* flags, const float* gscale, float w_policy, int B, int A, void* stream);
/* The policy cross-entropy against a distribution over at most 64 actions per row (the visit counts of a search): row b has
 * K slots (actions[b][k] int32, weights[b][k] fp32), 1 <= K <= 64.  A slot is used iff its weight is > 0; a slot of weight
 * 0 is ignored whatever its action.  One workgroup per row on ka_policy_ce's row pass (the row staged in LDS, the same
 * maximum, sum and lse).  With s = w_policy [* *gscale]:
 *   rowloss[b]    = sum_k w_k (lse - z[a_k])                       over the used slots, in slot order
 *   dlogits[b][j] = s (sum_k w_k) exp(z_j - lse) - s sum_{k: a_k = j} w_k      (optional; duplicate actions add in slot
 *                   order; an element some used slot names is fma(s W, exp(z_j - lse), -(s * its weights)))
 * flags[0] |= NaN in the logits.  flags[1] |= a used slot whose action lies outside [0, A), a weight that is negative or
 * not finite, or a row without a used slot: such a row gives rowloss 0 and a zero gradient row.  A row whose only used
 * slot has weight 1.0 gives, to the bit, the rowloss and the dlogits of ka_policy_ce with that action as its target. */
int ka_policy_ce_soft(const float* logits, const int* actions, const float* weights, int K, float* dlogits, float* rowloss,
                      int* flags, const float* gscale, float w_policy, int B, int A, void* stream);
int ka_value_loss(const float* vlogits, const float* score, const long long* cats, const float* targets,
                  const long long* idx, const float* rowloss, const float* rowent, float* dvlogits, float* dscore,
                  float* out, float* acc, const float* gscale, float lambda_policy, float lambda_value, float lambda_score,
                  float entropy_coeff, int combined_value_metric, int B, void* stream);
/* Held-out evaluation of one batch of the supervised heads: no gradient.  logits (B, A), vlogits (B, 3), score (B) and the
 * targets policy_t / value_t (int64) and score_t (fp32), row b of each.  The batch is ADDED into acc, 64 bytes, 8-byte aligned,
 * zeroed by the caller before the first batch:
 *   int64   [positions, top1, topk, value_correct]
 *   float64 [sum of policy CE, sum of value CE, sum of squared score error, 0]
 * sums over positions, so batches of different sizes weigh what they should.  Per row: policy CE = logsumexp(z) - z_t in
 * fp32 as ka_policy_ce forms it; rank = #{j : z_j > z_t} + #{j < t : z_j == z_t}, the target's place in a stable descending
 * sort, top1 = (rank == 0), topk = (rank < k), 1 <= k <= A; value CE and the predicted class by ka_value_loss's rule
 * (l0 >= l1 && l0 >= l2 ? 0 : l1 >= l2 ? 1 : 2).  A policy target outside [0, A) adds nothing to the policy terms, a value
 * target outside {0, 1, 2} nothing to the value terms; either sets flags[1].  flags[0] |= NaN in the logits, the value logits
 * or the score.  rowloss (fp32[B]) and rank (int32[B]) are workspace.  All reductions run in a fixed order: the same input
 * gives the same bits. */
int ka_sl_eval(const float* logits, const float* vlogits, const float* score, const long long* policy_t,
               const long long* value_t, const float* score_t, int B, int A, int k, float* rowloss, int* rank, void* acc,
               int* flags, void* stream);
/* P(W) - P(L), optionally blended with clamp(score,-1,1) (katago_ppo.py:533-541, value_adapter.py:76-96) */
int ka_scalar_value(const float* vlogits, const float* score, float alpha, float* out, int B, void* stream);

/* ---- GradScaler.unscale_ + clip_grad_norm_ + torch.optim.Adam.step + GradScaler.update (katago_ppo.py:926-933) --
 * tab: nt records {float* p, const float* g, float* m, float* v, long long n}; blk_tensor / blk_off map each of the
 * nblocks chunks (ka_adam_chunk() elements) to (record, element offset).  ctl[0] = unscaled global grad norm,
 * ctl[2] = 1 when the step was vetoed (inf/NaN gradients or a guard flag); step_state[0] = applied steps;
 * scaler = {scale, growth_tracker} or NULL. */
int ka_adam_chunk(void);
int ka_clip_adam_step(const void* tab, const int* blk_tensor, const long long* blk_off, int nblocks, double* partial,
                      float* ctl, float* step_state, float* scaler, const int* guard_flags, float* acc_gnorm,
                      float max_norm, float lr, float beta1, float beta2, float eps, void* stream);

/* ---- Generalised Advantage Estimation (gae.py:8-296) and advantage normalisation (katago_ppo.py:797-798) --
 * (T,N) grids, one launch; override: NaN = default bootstrap; lengths (N) selects the padded variants;
 * f64 != 0: rewards/values/next_value/override/adv are double.  Bit-identical to compute_gae_gpu's op order. */
int ka_gae(const void* rewards, const void* values, const float* term, const void* next_value, const void* override_,
           const long long* lengths, void* adv, int T, int N, double gamma, double lam, int f64, void* stream);
int ka_normalize_advantages(const float* x, float* out, long long n, void* stream);

/* ---- Device-resident rollout store (KataGoRolloutBuffer.add / flatten, katago_ppo.py:128-388) --
 * ka_rollout_append: one timestep of n transitions.  Sources are the tensors add() receives (obs fp32 (n,obs_elems),
 *   legal bool (n,A), actions / cats / env_ids int64, log_probs / values / rewards / score / override fp32, dones /
 *   terminated bytes); destinations are the store's columns already offset to the first row written; the mask row
 *   is packed to ka_mask_words(A) uint32 (bit j of word w = action 32 w + j).  env_ids / override / d_env_ids /
 *   d_override may be NULL; a store with an override column and no override supplied gets NaN (= no override).
 *   The reference's input guards (katago_ppo.py:244-266) come back as flags: [0] terminated without done,
 *   [1] category outside {-1,0,1,2}, [2] NaN score target, [3] = float bits of max |score target| seen.
 * ka_unpack_mask_bits: bool rows out[r] = packed row idx[r] (idx NULL = identity) -- flatten()'s legal_masks.
 * ka_pack_mask_bits: packed rows from bool rows. */
int ka_mask_words(int A);
int ka_rollout_append(const float* obs, const void* legal, const long long* actions, const float* log_probs,
                      const float* values, const float* rewards, const void* dones, const void* terminated,
                      const long long* cats, const float* score, const long long* env_ids, const float* override_,
                      float* d_obs, void* d_bits, long long* d_actions, float* d_log_probs, float* d_values, float* d_rewards,
                      void* d_dones, void* d_terminated, long long* d_cats, float* d_score, long long* d_env_ids,
                      float* d_override, int* flags, int n, int obs_elems, int A, void* stream);
/* as ka_rollout_append with the legal masks already PACKED: legal_bits (n, ka_mask_words(A)) uint32 rows (the device env's
 * StepResult.legal_mask_bits, PendingTransitions.finalize()["legal_mask_bits"]) are copied word for word. */
int ka_rollout_append_packed(const float* obs, const void* legal_bits, const long long* actions, const float* log_probs,
                             const float* values, const float* rewards, const void* dones, const void* terminated,
                             const long long* cats, const float* score, const long long* env_ids, const float* override_,
                             float* d_obs, void* d_bits, long long* d_actions, float* d_log_probs, float* d_values, float* d_rewards,
                             void* d_dones, void* d_terminated, long long* d_cats, float* d_score, long long* d_env_ids,
                             float* d_override, int* flags, int n, int obs_elems, int A, void* stream);
int ka_unpack_mask_bits(const void* bits, const long long* idx, void* out, int rows, int A, void* stream);
int ka_pack_mask_bits(const void* legal, void* bits, int rows, int A, void* stream);

/* ---- Pending learner transitions of the split-merge rollout (PendingTransitions.create / accumulate_reward / finalize,
 * katago_loop.py:139-250).  Slots = one row per game: obs fp32 (n, obs_elems), legal masks PACKED (n,
 * ka_mask_words(A)) uint32, actions int64, log_probs / values / rewards / score fp32, valid bytes.
 * ka_pending_open (create(), katago_loop.py:172-200): the games with env_mask != 0 take this step's rows; masks come as bool
 *   rows (s_legal, (n, A)) and are packed on the way, or as packed rows (s_bits) and are copied.  flags[0] = 1 and nothing is
 *   written when a selected slot still holds a transition (the reference's RuntimeError).
 * ka_pending_accumulate (accumulate_reward(), :203-211): rewards[valid] += add[valid].
 * ka_pending_settle (finalize(), :213-250): rows of the games with fin_mask & valid, in game order, into the o_* columns
 *   (n rows allocated; flags[1] = rows written); dones / terminated are this step's flags for all n games, floats
 *   (flags_are_f32 != 0) or bytes; add_rewards (may be NULL) is accumulated first, as accumulate_reward() would; o_cats =
 *   the value-head labels of _compute_value_cats (:75-92) for the settled rows; settled slots are released (valid_out, a
 *   second buffer: the launch still counts over `valid`) and their rewards zeroed. */
int ka_pending_open(float* obs, void* bits, long long* actions, float* log_probs, float* values, float* rewards, float* score,
                    void* valid, const void* env_mask, const float* s_obs, const void* s_legal, const void* s_bits,
                    const long long* s_actions, const float* s_log_probs, const float* s_values, const float* s_rewards,
                    const float* s_score, int* flags, int n, int obs_elems, int A, void* stream);
int ka_pending_accumulate(float* rewards, const void* valid, const float* add_rewards, int n, void* stream);
int ka_pending_settle(float* obs, void* bits, long long* actions, float* log_probs, float* values, float* rewards, float* score,
                      const void* valid, void* valid_out, const void* fin_mask, const void* dones, const void* terminated,
                      int flags_are_f32, const float* add_rewards, float* o_obs, void* o_bits, long long* o_actions,
                      float* o_log_probs, float* o_values, float* o_rewards, float* o_dones, float* o_terminated, float* o_score,
                      long long* o_env_ids, long long* o_cats, int* flags, int n, int obs_elems, int A, void* stream);

/* ---- the eval-mode residual tower in one launch (rollout inference, SURVEY 8 f2: katago_ppo.py:543-617 calling
 * se_resnet.py:67-75 for every block under no_grad / eval()).  One workgroup carries one board through all blocks; the
 * activations live in LDS.  x_in / x_out (B, 81, C) bf16, pool_in / pool_out (B, 4C) fp32 [mean|max|std|-]; blocks = device
 * table of nblocks rows of 14 pointers: {conv1 pack, conv2 pack (ka_pack_conv3x3 mode 0), bn1 scale, bn1 shift, bn2 scale,
 * bn2 shift (eval), global_fc[0].weight (G,3C), .bias, global_fc[2].weight (C,G), .bias, se_fc1.weight (R,C), .bias,
 * se_fc2.weight (2C,R), .bias}. */
int ka_tower_eval_supported(int C, int G, int R, int dtype);
int ka_tower_eval(const void* x_in, const float* pool_in, void* x_out, float* pool_out, const void* blocks, int nblocks, int B,
                  int C, int G, int R, int dtype, void* stream);
/* ---- grouped eval forward: many SE-ResNets of one shape over one board batch (league / tournament play: the reference's
 * concurrent_matches.py:353-364 one forward per resident model, katago_loop.py:404-431 one forward per cohort opponent).
 * Board b runs model model_of[b] (int32); a board whose index lies outside [0, K) is unseated: it reads no weights and its
 * outputs are zeros.  Eval mode, bf16 activations, C in {128, 256}; three launches whatever K is, no host synchronisation. */
int ka_tower_eval_grouped_supported(int C, int G, int R, int dtype);
/* se_resnet.py:101 relu(input_bn(input_conv(obs))) per board: obs (B, cin, 9, 9) fp32 (cin <= 128); x_out (B, 81, C) bf16,
 * pool_out (B, 4C) [mean|max|std|0] as ka_tower_eval reads them; stems = device table of K rows of 3 pointers {input_conv
 * pack (ka_pack_conv3x3 mode 0, Kin = 128), input_bn eval scale, shift}. */
int ka_stem_eval_grouped(const float* obs, const int* model_of, const void* stems, int K, void* x_out, float* pool_out, int B,
                         int cin, int C, int dtype, void* stream);
/* se_resnet.py:67-75 x num_blocks with a model per board: ka_tower_eval over tables = device table (K, nblocks, 14) of
 * TowerBlock rows (the ka_tower_eval layout, one set of blocks per model). */
int ka_tower_eval_grouped(const void* x_in, const float* pool_in, void* x_out, float* pool_out, const int* model_of,
                          const void* tables, int K, int nblocks, int B, int C, int G, int R, int dtype, void* stream);
/* se_resnet.py:102-106 heads per board: logits (B, 9, 9, 139) = policy_conv2(relu(policy_bn1(policy_conv1(x)))), value
 * (B, 3) = value_fc2(relu(value_fc1(pool))), score (B, 1) = score_fc2(relu(score_fc1(pool))), all fp32, from the tower's
 * x (B, 81, C) bf16 and pool (B, 4C); heads = device table of K rows of 13 pointers {policy_conv1.weight (P, C), policy_bn1
 * eval scale, shift, policy_conv2.weight (139, P), .bias, value_fc1.weight, .bias, value_fc2.weight, .bias, score_fc1.weight,
 * .bias, score_fc2.weight, .bias}.  P <= 32, V, S <= 512. */
int ka_heads_eval_grouped(const void* x, const float* pool, const int* model_of, const void* heads, int K, float* logits,
                          float* value, float* score, int B, int C, int P, int V, int S, int dtype, void* stream);

/* ---- the vectorised shogi environment on the device (shogi-engine/crates/shogi-gym/src/vec_env.rs:556-855
 * VecEnv(num_envs, max_ply, "katago", "spatial"), with the rules of shogi-core/src/{movegen,attack,rules,game}.rs, the
 * observation planes of shogi-gym/src/katago_observation.rs:41-92 + observation.rs:81-153 and the action indices of
 * spatial_action_mapper.rs:138-279).  One wave per game; all buffers are device memory owned by the caller:
 *   state  n x ka_shogi_env_state_bytes() bytes: board[81] (piece.rs:10-19 bytes) hands[2][7] side in_check - ply key reps games
 *   keys   n x max(max_ply,1) u64, checks n x max(max_ply,1) u8: position key / "mover stood in check" of every ply
 *   obs_mode 1 = "katago" 50 planes, 0 = "default" 46 planes (observation.rs:1-15); action_mode 1 = "spatial" A = 11 259,
 *   0 = "default" A = 81*80*2 + 81*7 = 13 527 (action_mapper.rs:17-110); ka_shogi_env_action_space(mode) = A.
 *   obs (n,planes,9,9) fp32; mask (n,A) bool bytes and/or mask_bits (n,ceil(A/32)) u32 (bit j of word w = action 32w+j;
 *   at least one of the two); current_players (n) u8.
 * ka_shogi_env_reset: VecEnv::reset (vec_env.rs:617-645) -- or, with refresh != 0, derive key / check / masks from the
 *   board, hands and side the caller has written into `state` (test fixtures; ply and history start at 0).
 * ka_shogi_env_step: VecEnv::step (vec_env.rs:651-700, apply_moves :340-460).  Phase 1 checks every action against
 *   prev_mask / prev_mask_bits (the masks of the previous call); `err` points at FOUR ints = two 64-bit words, 8-byte aligned:
 *   word 0 (cleared by every call) = ((n - i) << 32) | (uint32) action for the first refused env i, and then NO game moves (the
 *   reference raises before mutating); word 1 latches the first non-zero word 0 and is never cleared by the library: the
 *   caller zeroes it when it has reported the refusal, so a flag read late survives any number of further steps.  Phase 2: make_move, check_termination (game.rs:355-387: move
 *   limit, fourfold repetition / perpetual check, 24-point impasse, no legal move), rewards for the mover
 *   (vec_env.rs:98-124), captured hand-type (255 none), TerminationReason, ply, material balance, episode counters
 *   stats[4] u64 {completed, drawn, truncated, total ply}; finished games write terminal_obs (other rows are left as they
 *   were) and restart from the start position; then observation and masks of every game's position to move.
 * ka_shogi_env_reset_pool / ka_shogi_env_step_pool: the same calls with a pool of start positions, replacing the standard
 *   start of reset and of every restart (the reference has no counterpart: VecEnv always starts at position.rs:45-93).
 *   pool = capacity rows of 96 bytes board[81] hands[2][7] side (the first 96 bytes of a state row), pool_hdr = int32[4]
 *   {count, 0, seed lo, seed hi}, both device memory.  Every launch reads count (<= capacity, the caller's promise) and the
 *   seed from the header, so new contents apply from the next ply of a captured graph.  A game starting in env e draws
 *     h = mix(seed ^ mix(((u64)e << 32 | g) + 0x706F6F6C)),  idx = ((h >> 32) * count) >> 32,  mix = the splitmix64 finaliser,
 *   with g = games started in e since the last reset (u32 at byte 116 of the state row: reset writes 0, a restart adds 1,
 *   refresh leaves it; the game ply, the ply of the position to move in, is the u32 at byte 100), and starts from row idx with ply 0, an empty history, repetition count 1, in_check and key derived.
 *   The rows must be playable positions (keisei_amd.shogi_gym validates them).  count <= 0 or pool = pool_hdr = NULL is
 *   the standard start: exactly ka_shogi_env_reset / ka_shogi_env_step, which never touch byte 116. */
int ka_shogi_env_state_bytes(void);
int ka_shogi_env_action_space(int action_mode);
int ka_shogi_env_reset(void* state, void* keys, void* checks, int n, int max_ply, int obs_mode, int action_mode, float* obs,
                       void* mask, void* mask_bits, void* current_players, int refresh, void* stream);
int ka_shogi_env_step(void* state, void* keys, void* checks, const long long* actions, int n, int max_ply, int obs_mode,
                      int action_mode, const void* prev_mask, const void* prev_mask_bits, int* err, float* obs, void* mask, void* mask_bits,
                      float* rewards, void* terminated, void* truncated, float* terminal_obs, void* current_players,
                      void* captured, void* term_reason, void* ply_count, int* material, void* stats, void* stream);
int ka_shogi_env_reset_pool(void* state, void* keys, void* checks, int n, int max_ply, int obs_mode, int action_mode, float* obs,
                            void* mask, void* mask_bits, void* current_players, int refresh, const void* pool,
                            const void* pool_hdr, void* stream);
int ka_shogi_env_step_pool(void* state, void* keys, void* checks, const long long* actions, int n, int max_ply, int obs_mode,
                           int action_mode, const void* prev_mask, const void* prev_mask_bits, int* err, float* obs, void* mask,
                           void* mask_bits, float* rewards, void* terminated, void* truncated, float* terminal_obs,
                           void* current_players, void* captured, void* term_reason, void* ply_count, int* material,
                           void* stats, const void* pool, const void* pool_hdr, void* stream);

/* ---- match arena (csrc/arena.hip; concurrent_matches.py:196-545 run_round): S slots of E contiguous envs, slot s playing
 * model_a (player 0) against model_b (player 1).  state: ka_arena_state_words(S) int32 = header {seed int64, round ply,
 * ceiling max_ply, sampler flags[2], refusal latch copy int64} + S x {model_a, model_b, target, a_wins, b_wins, draws, plies, status}, status
 * bits 1 seated, 2 done, 4 partial, 8 stalled.  model_of (S*E) int32, pre_player (S*E) u8.
 * ka_arena_referee (after ka_shogi_env_step): tallies the finished games of every seated, unfinished slot by the last-mover
 * rule, closes slots at their target (overshoot counted), at the ply ceiling state max_ply * (ceil(target / E) + 1) (partial) or
 * when a seated env had nlegal == 0 (target = games so far), writes the next ply's model_of / pre_player from the new
 * current players (-1 for idle or finished slots), advances the seed and the round ply and copies *refusal (may be NULL).
 * ka_arena_assign: jobs = njobs rows {slot, model_a, model_b, target}: seat the pairing, zero the slot's counters and seat
 * its envs from the current players. */
int ka_arena_state_words(int slots);
int ka_arena_referee(int* state, int slots, int envs_per_slot, const float* rewards, const void* terminated,
                     const void* truncated, const void* players, const int* nlegal, const long long* refusal, int* model_of,
                     void* pre_player, void* stream);
int ka_arena_assign(int* state, const int* jobs, int njobs, int envs_per_slot, const void* players, int* model_of,
                    void* pre_player, void* stream);
/* Rollout collection inside the ply (concurrent_matches.py:80-163 the per-slot _obs / _masks / _perspective / _actions /
 * _rewards / _dones lists, :318-327, :366-372, :421-432 the appends).  The store holds `cap` rows per slot (row r of slot s
 * is store row s * cap + r): st_obs (S*cap, obs_elems) fp32, st_mask_bits (S*cap, mask_words) uint32, st_actions int64,
 * st_perspective u8, st_rewards / st_dones fp32.  cursors: ka_arena_cursor_words(S) int32 = S x {rows committed, rows written
 * this ply, rows dropped, unused}; row_of (S*E) int32 = the store row of each env's row of this ply, -1 = none.
 * side_bits (S) int32: bit 0 = collect side A's rows (pre-step player 0), bit 1 = side B's.
 * ka_arena_record_pre (after ka_policy_sample_play, before ka_shogi_env_step): for every slot that is seated, not done, has
 *   side bits and no env with nlegal == 0 (:303-314), appends one row per env whose mover is on a collected side, in env order,
 *   behind the rows committed so far; rows beyond cap are not written and are counted as dropped.  No atomics: the order
 *   inside a slot is (ply, env).
 * ka_arena_record_post (after ka_shogi_env_step, before ka_arena_referee): writes rewards and dones = terminated | truncated
 *   (fp32 0 / 1, :427-432) into this ply's rows and commits them.
 * The host reads and zeroes `cursors` at its sync point, outside any captured graph. */
int ka_arena_cursor_words(int slots);
int ka_arena_record_pre(const int* state, const int* side_bits, int slots, int envs_per_slot, const float* obs,
                        const void* mask_bits, const long long* actions, const void* pre_player, const int* nlegal,
                        int* cursors, int* row_of, float* st_obs, void* st_mask_bits, long long* st_actions,
                        void* st_perspective, int cap, int obs_elems, int mask_words, void* stream);
int ka_arena_record_post(int* cursors, const int* row_of, int slots, int envs_per_slot, const float* rewards,
                         const void* terminated, const void* truncated, float* st_rewards, float* st_dones, int cap,
                         void* stream);
/* Per-game style features inside the ply (game_feature_tracker.py:176-356 GameFeatureTracker; concurrent_matches.py:125-130
 * one tracker per seated pairing, :441-452 record_step on every stepped ply, :46 / :162 MatchResult.feature_tracker).
 * ka_arena_feature_words(which): int32 words of 0 = one env's accumulator {opening actions kept, num_repetitions, 12 opening
 *   actions, side A, side B}, 1 = one game record {env, total plies, termination reason, last mover, reward sign, opening
 *   actions kept, num_repetitions, round ply, 12 opening actions, side A, side B}, 2 = one slot's cursor {records committed,
 *   records dropped}; -1 for any other `which`.  A side is the ten _SideStats counters in their order (:67-80), -1 for None.
 * ka_arena_features_step (after ka_shogi_env_step, before ka_arena_referee, which rewrites status and pre_player): for every
 *   slot that is seated, not done and has no env with nlegal == 0 (concurrent_matches.py:303-314, :410), record_step
 *   (:204-284) on each env from its action, mover, captured (u8, 255 none), reason (u8), ply (uint16 payload) and, where
 *   terminated | truncated, _emit_game (:286-356): one record at records[s * cap + committed + rank], rank = the env's place
 *   among the slot's finished envs of this ply (no atomics: the order inside a slot is (ply, env)), and a fresh accumulator.
 *   Records beyond cap are not written and are counted as dropped.  acc (S*E x words(0)), records (S*cap x words(1)),
 *   fcursors (S x words(2)) int32.
 * ka_arena_features_seat (behind ka_arena_assign, same jobs): a fresh accumulator for every env of each job's slot (a new
 *   tracker per pairing, concurrent_matches.py:125); rows naming a slot outside [0, slots) are skipped.
 * The host reads and zeroes `fcursors` at its sync point, outside any captured graph. */
int ka_arena_feature_words(int which);
int ka_arena_features_step(const int* state, int slots, int envs_per_slot, const long long* actions, const void* pre_player,
                           const int* nlegal, const void* captured, const void* reason, const void* ply, const float* rewards,
                           const void* terminated, const void* truncated, int* acc, int* records, int* fcursors, int cap,
                           void* stream);
int ka_arena_features_seat(const int* jobs, int njobs, int slots, int envs_per_slot, int* acc, void* stream);
/* Dynamic-entry targets (dynamic_trainer.py:310-318, :358): cats[i] = 0 / 1 / 2 (win / draw / loss by the sign of rewards[i])
 * where dones[i] != 0, else -1; adv[i] = rewards[i] * dones[i]. */
int ka_dynamic_targets(const float* rewards, const float* dones, long long* cats, float* adv, long long n, void* stream);

/* ---- league rollout (csrc/league.hip; katago_loop.py:1162-1437 the opponent branch of the rollout loop, :1537-1563 the
 * flush at the end of an epoch).  E envs; the learner is model 0 of the group, opponent k (0 <= k < K) model k + 1.
 * state: ka_league_state_words K int32 = {0-1 sampler seed int64, 2 plies, 3 rows written behind the descriptor's base row,
 *   4 non-empty blocks (the reference's add() calls), 5 rows dropped, 6-7 sampler flags, 8-9 refusal latch copy int64,
 *   10-11 draw seed int64, 12 truncation slots used, 13 truncation records dropped, 14-20 wins / losses / draws (learner
 *   frame) / black wins / white wins / terminated / truncated-only, 21-24 the four guards of ka_rollout_append over the rows
 *   written, 25 a pending slot opened while taken, 26 zero-legal bits (1 learner row, 2 opponent row), 27-31 unused,
 *   then K x {wins, losses, draws}}.
 * ka_league_layout gives the other sizes: which 0 = int32 words of one env's plan, 1 = int64 words of the descriptor,
 *   2 = int32 columns of the pending scalars {action, log-prob, value, reward, score target, valid} (each E words, column
 *   major), 3 = int32 words of one truncation record {env, store row, player to move | learner side << 1}, 4 = largest E.
 * desc: {observations, legal mask bits, actions, log_probs, values, rewards, dones u8, terminated u8, value_categories,
 *   score_targets, env_ids, next_value_override} column base pointers of the rollout store, the base row and the number of
 *   rows reserved behind it.  It is read on the device by every launch, so a captured graph survives a store that grows:
 *   the host rewrites it at its sync points.
 * ka_league_step, after ka_shogi_env_step, with flush = 0: one ply's bookkeeping in the reference's order --
 *   (1) learner-frame rewards: the reward of a ply the opponent moved is negated (to_learner_perspective, :111-122), and the
 *   tallies of :1219-1248; (2) rewards accumulate into the pending slots and the slots with valid & (done | learner to move
 *   next) settle (:1290-1316) as rows of the store in env order, labelled by _compute_value_cats (:75-92); (3) a slot opens
 *   where the learner moved (:1319-1341): pre-step observation and packed mask, action, log-prob, value P(W) - P(L) blended
 *   with clamp(score_lead, -1, 1) by alpha as ka_policy_sample does, reward, score target material / score_norm; (4) where
 *   that move ended the game it settles at once, a second block of rows behind the first (:1343-1365); (5) terminated games
 *   count for the opponent that played them (:1384-1407); (6) every done env draws its next opponent and (7), with
 *   color_rand, its next learner side (:1409-1437); (8) model_of of the next ply.  Rows of truncated, unterminated games
 *   (:1250-1283) put the env's terminal observation into a truncation slot with a record; the host computes the bootstrap
 *   override there.  Rows beyond the reserved capacity are not written and are counted.  values[e] = the learner's value
 *   where it moved, else 0.  stall (E) u8 latches the zero-legal bits per env.  No atomics: rows are ranked by ballot scans.
 *   flush = 1 (:1537-1563): every pending slot settles with done = terminated = 0, label -1; the step's tensors are unused.
 * Draws: mix = the splitmix64 finaliser x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *   x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31.  h(salt, env, n) = mix(draw_seed ^ mix((env << 32 | n) + salt)), n = the
 *   games that env has finished since the reset, this one included.  opponent = the first k with
 *   h(0x6F70706F, env, n) >> 33 < cum[k] (K uint32 thresholds of the cumulative weights on a 31-bit scale, the last one
 *   2^31); side = h(0x73696465, env, n) >> 63. */
int ka_league_state_words(int opponents);
int ka_league_layout(int which);
int ka_league_step(int* state, int envs, int opponents, int flush, const float* obs, const void* mask_bits,
                   const long long* actions, const float* logp, const float* vlogits, const float* score_lead, float alpha,
                   const int* nlegal, const void* pre_player, const float* rewards, const void* terminated,
                   const void* truncated, const void* players, const int* material, float score_norm, const float* term_obs,
                   const long long* refusal, void* side, int* opp, int* games, const void* cum, int color_rand,
                   int* model_of, void* stall, float* values, float* p_obs, void* p_bits, int* p_scal, float* t_obs,
                   int* t_list, const long long* desc, int* plan, int obs_elems, int mask_words, void* stream);

/* ---- self-play rollout (csrc/selfplay.hip; katago_loop.py:1438-1527, the no-opponent branch of the rollout loop: every
 * env is the learner, every ply gives one transition per env).  E envs, one model.
 * state: ka_selfplay_state_words() int32 = {0-1 sampler seed int64, 2 ply of the epoch, 3 rows written behind the
 *   descriptor's base row, 4 plies since the reset, 5 rows dropped, 6-7 sampler flags, 8-9 refusal latch copy int64, 10-11
 *   unused, 12 truncation slots used, 13 truncations without a slot, 14-20 wins / losses / draws (the mover's frame) / black
 *   wins / white wins / terminated / truncated-only, 21-24 the four guards of ka_rollout_append over the rows written, 25 an
 *   env without a legal action, 26-31 unused}.
 * ka_selfplay_layout gives the other sizes: which 0 = int32 words of one env's plan {store row, truncation slot}, 1 = int64
 *   words of the descriptor, 2 = int32 words of one truncation record {env, store row}, 3 = largest E.
 * desc: the league rollout's descriptor; the env_ids pointer is not read (the dense (T, N) layout has no such column).
 * ka_selfplay_step, after ka_shogi_env_step: env e at ply p = state[2] owns store row base + p * E + e; a row beyond the
 *   reserved capacity is not written and is counted.  Statement by statement:
 *     :1446       values[e] = the learner's value this ply (latest_values)
 *     :1455-1458  rewards in the mover's frame, done = terminated | truncated
 *     :1460-1461  terminated and truncated-only counts
 *     :1463-1485  wins / losses / draws by the sign of the reward over terminated envs, black / white wins by pre_player
 *     :1487       label {-1, 0, 1, 2} (_compute_value_cats, :75-92)
 *     :1491-1494  score target material / score_norm
 *     :1502-1521  a truncated, unterminated env parks terminal_observations[e] in a truncation slot with {env, store row},
 *                 slots in (ply, env) order; the host computes -V there at its sync point.  next_value_override = NaN
 *     :1523-1527  the row: pre-step observation and packed mask row, action, log-prob, value P(W) - P(L) blended with
 *                 clamp(score_lead, -1, 1) by alpha (the arithmetic of ka_policy_sample), reward, done, terminated, label,
 *                 score target; the add() guards become state words 21-24
 *   stall (E) u8 latches the envs without a legal action.  The seed advances by the Weyl step 0x9E3779B97F4A7C15 and
 *   state[2] by one per call, so a captured graph replays.  No atomics: truncation slots are ranked by ballot scans. */
int ka_selfplay_state_words(void);
int ka_selfplay_layout(int which);
int ka_selfplay_step(int* state, int envs, const float* obs, const void* mask_bits, const long long* actions,
                     const float* logp, const float* vlogits, const float* score_lead, float alpha, const int* nlegal,
                     const void* pre_player, const float* rewards, const void* terminated, const void* truncated,
                     const int* material, float score_norm, const float* term_obs, const long long* refusal, void* stall,
                     float* values, float* t_obs, int* t_list, const long long* desc, int* plan, int obs_elems,
                     int mask_words, void* stream);

/* ---- game log (csrc/gamelog.hip; the per-env move_history of the reference's VecEnv, vec_env.rs:259, cleared on
 * auto-reset): the moves of the games played on the device, kept inside the ply and handed over as whole finished games.
 * E envs (at most ka_gamelog_words(6, 0)); every buffer is device memory owned by the caller:
 *   rows     E x row_stride uint16, 4-byte aligned, row_stride even and >= max_ply: the moves of the game in progress
 *   meta     E x ka_gamelog_words(2, 0) int32 {moves in the row, carried (0 / 1), games finished since begin, player tag
 *            (ka_gamelog_step_env only: 0 for an empty row, else the tag of the players who made the row's last move)}
 *   starts   E x 24 int32: the first 96 bytes of the env's state row (board[81] hands[2][7] side, a pool row) as they were
 *            when the game in progress began
 *   records  game_cap x ka_gamelog_words(0, max_ply) int32, one finished game each: 12 header words {env, plies, winner
 *            0 black / 1 white / 2 draw, termination reason, flags (bit 0 truncated and not terminated, bit 1 carried),
 *            black id, white id, the owner's ply counter, number of the game within its env since begin, the learner's
 *            colour + 1 (1 black, 2 white; 0 = no learner, what ka_gamelog_step writes), 2 zero words},
 *            the 24 start words, then the moves two per word, low half first.  The unused half of the last move word is
 *            zero; the words behind it are not written.
 *   cursor   ka_gamelog_words(1, 0) int32 {records committed, records dropped, plies logged, unused}.  The host reads and
 *            zeroes it at its sync point, outside any captured graph.
 * ka_gamelog_words(which, max_ply): int32 words of 0 = one record, 1 = the cursor, 2 = one env's meta, 3 = the move words
 *   of a record ((max_ply + 1) / 2), 4 = a record's header, 5 = a start position; 6 = the largest E; -1 for any other which.
 * ka_gamelog_begin (after ka_shogi_env_reset / ka_shogi_env_reset_pool): for every env an empty row, carried 0, game
 *   number 0, player tag 0, and the start slot copied from the state row (state_bytes = ka_shogi_env_state_bytes(), a
 *   multiple of 4).
 * ka_gamelog_step (after ka_shogi_env_step / ka_shogi_env_step_pool, BEFORE the owner's bookkeeping launch --
 *   ka_selfplay_step, ka_arena_referee -- because the referee rewrites model_of and pre_player).  For every env e, in
 *   this order:
 *     1. actions[e] is appended to the row as uint16 unless the row already holds max_ply moves (it then stays as it is).
 *     2. live (E int32, may be NULL = every env is live; the arena's pre-step model_of): where live[e] < 0 the env's carried
 *        flag is set -- a ply of this game was not played by a seated model.
 *     3. where terminated[e] | truncated[e], the env is live, and no env of its group had nlegal == 0 (nlegal may be
 *        NULL; the group of e is the envs_per_pair envs of pair e / envs_per_pair when pairs is given, else e alone:
 *        the rule by which ka_arena_referee leaves a stalled slot untallied), the game is committed as one record:
 *        plies = the moves in the row, winner from the sign of rewards[e] (the mover's reward) and pre_player[e] (u8, the
 *        mover): positive -> the mover, negative -> the other side, zero or NaN -> draw (the outcome of
 *        ka_sl_replay_record); reason = term_reason[e] (u8); black / white = pairs[(e / envs_per_pair) * pair_stride + 0 / 1]
 *        (the arena passes its slot table: model_a plays black, model_b white) or -1 when pairs is NULL; the owner's
 *        ply counter = *ply_counter as this launch finds it (0 when NULL).
 *     4. for every env that finished, live or not: the row is emptied, carried cleared, the game number advanced and the
 *        start slot reloaded from the state row, where the env kernel has already restarted the game (from the standard
 *        start or the pool row it drew).
 *   Records are written behind the committed ones in (ply, env) order: the rank of a committed env is its place among the
 *   committed envs of this ply in env order (ballot scans in one workgroup that walks the envs in tiles of 256; no
 *   atomics, nothing waits on another workgroup), so the order does not depend on the launch geometry.  A game that does
 *   not fit game_cap is dropped whole and counted; nothing is written outside the buffers named above.
 *   ka_gamelog_step neither reads nor writes the fourth meta word.
 * ka_gamelog_step_env (the league rollout: after ka_shogi_env_step, BEFORE ka_league_step, which re-draws side and opp of
 *   the envs that finished -- so it reads the players who played the ply): ka_gamelog_step with per-env players in place
 *   of the pair table.  The group of an env is the env itself.  side (E u8): the learner's colour in env e, 0 black (bit
 *   0 is read); opp (E int32): the opponent index k of env e; ids (opponents + 1 int32, device memory): ids[0] the
 *   learner's id, ids[k + 1] opponent k's.  Steps 1-4 as above, the same kernel body, with these differences:
 *     - black / white of a record = ids[0] on the learner's side, ids[opp[e] + 1] on the other; an opp[e] outside
 *       [0, opponents) gives -1 and reads nothing outside ids.  Header word 9 = side[e] + 1.
 *     - tag = ((opp[e] << 1) | side[e]) + 1 in 32-bit wrapping arithmetic.  Where the row was empty before step 1 the
 *       fourth meta word becomes tag; where it held a move and the word differs from tag, the carried flag is set (before
 *       step 3, so a record carries it) and the word becomes tag: a side or an opponent re-drawn on the host or on the
 *       device in the middle of a game needs no call here, and the record names the players who ended the game, the ones
 *       ka_league_step tallies it for.  A change between two games sets nothing.  Where the game finished the word becomes 0.
 * ka_gamelog_peek (at a sync point; not meant for capture): the games in progress.  Writes n record-shaped rows of
 *   ka_gamelog_words(0, max_ply) words into out, row j for env envs_list[j] (n int32, device memory), or env j when
 *   envs_list is NULL (then n <= envs); one wave per row.  Header {env, moves in the row, -1, 0, flags = the carried bit
 *   alone, black, white, *ply_counter (0 when NULL), game number, learner's colour + 1, 0, 0}, the 24 start words, the moves
 *   two per word with the unused half of the last word zero; the words behind are not written.  Players: from pairs
 *   (pair_stride, envs_per_pair) as ka_gamelog_step names them; or from side / opp / ids / opponents as
 *   ka_gamelog_step_env names them (word 9 = side + 1); giving both is an error; with neither black = white = -1 and
 *   word 9 = 0.  An index outside [0, envs) gives env -1, 0 moves, players -1, zero start words and reads no env buffer.
 *   rows, meta and starts are only read; records and cursor are not touched.
 * ka_gamelog_seat (behind ka_arena_assign, same jobs = njobs rows of 4 int32 {slot, ...}): every env of a job's slot whose
 *   row holds a move gets carried = 1 (the new pairing inherits that game); a slot outside [0, slots) is skipped. */
int ka_gamelog_words(int which, int max_ply);
int ka_gamelog_begin(const void* env_state, int state_bytes, int envs, int* meta, int* starts, void* stream);
int ka_gamelog_step(const void* env_state, int state_bytes, int envs, int max_ply, const long long* actions,
                    const float* rewards, const void* terminated, const void* truncated, const void* pre_player,
                    const void* term_reason, const int* nlegal, const int* live, const int* pairs, int pair_stride,
                    int envs_per_pair, const int* ply_counter, void* rows, int row_stride, int* meta, int* starts,
                    int* records, int game_cap, int* cursor, void* stream);
int ka_gamelog_step_env(const void* env_state, int state_bytes, int envs, int max_ply, const long long* actions,
                        const float* rewards, const void* terminated, const void* truncated, const void* pre_player,
                        const void* term_reason, const int* nlegal, const int* live, const void* side, const int* opp,
                        const int* ids, int opponents, const int* ply_counter, void* rows, int row_stride, int* meta,
                        int* starts, int* records, int game_cap, int* cursor, void* stream);
int ka_gamelog_peek(const int* envs_list, int n, int envs, int max_ply, const int* pairs, int pair_stride, int envs_per_pair,
                    const void* side, const int* opp, const int* ids, int opponents, const int* ply_counter,
                    const void* rows, int row_stride, const int* meta, const int* starts, int* out, void* stream);
int ka_gamelog_seat(const int* jobs, int njobs, int slots, int envs_per_slot, int* meta, void* stream);

/* ---- spectator feed (csrc/spectator.hip; the move_histories of the reference's VecEnv, vec_env.rs:259, 618-622, 693-714,
 * with what its Hodges notation needs, spectator_data.rs:105-186).  Per env and move one uint32 note, computed on the
 * device from the position and the packed legal mask of the moment of the move; the host turns notes into text.
 * Note, from bit 0 (ka_spectator_words(which) gives the positions: 0 = bits of the action index, 14; then the shift of
 * 1 = colour, 2 = piece type, 3 = promoted, 4 = drop, 5 = capture, 6 = suffix, 7 = disambiguation, 8 = no piece; 9 = int32
 * words of one note; -1 for any other which):
 *   action index; the mover's colour (state byte 95); piece type (4 bits, 1 P 2 L 3 N 4 S 5 G 6 B 7 R 8 K: of the piece
 *   on `from`, or the dropped type); that piece is already promoted; drop; capture (a board move whose `to` is occupied);
 *   promotion suffix class (2 bits): 1 = '+' when the move promotes or must_promote(type, to row, colour) (movegen.rs:35-47,
 *   whatever the piece's promotion state), else 2 = '=' when the piece can promote, is unpromoted and `from` or `to` lies
 *   in the mover's zone, else 0; disambiguation class (2 bits): 0 none, 1 file, 2 rank, 3 full square; no piece on `from`
 *   (then type, promoted, suffix and disambiguation are 0).
 *   The "others" of the disambiguation are the squares other than `from` and `to` that hold the same piece byte as `from`
 *   and whose move to `to`, plain or promoting, is set in the mask row; a king is never disambiguated.
 *   An action outside [0, A) gives note 0 and reads neither the board nor the mask row; an action inside it that points
 *   off the board (spatial mode) gives the bare action index.  The env refuses both.
 * Buffers, device memory owned by the caller: pending envs x uint32; hist envs x row_len uint32 (row_len >= max_ply, so a
 *   row never fills before the env truncates the game); count envs x int32.
 * ka_spectator_begin: every count becomes 0 (after a reset, or after positions were placed).
 * ka_spectator_note (BEFORE ka_shogi_env_step / ka_shogi_env_step_pool, on its stream): one wave per env; env_state the
 *   state rows (state_bytes = ka_shogi_env_state_bytes()), mask_bits the packed rows the step validates against
 *   (prev_mask_bits), actions the step's actions, action_mode 0 default / 1 spatial.  Writes pending[e] only.
 * ka_spectator_commit (AFTER the env step): err the step's refusal words (err[0] != 0: the step was refused and nothing is
 *   written); otherwise pending[e] is appended at hist[e][count[e]] -- a row that already holds row_len notes stays as it
 *   is -- and count[e] becomes 0 where terminated[e] | truncated[e] (u8 each, the step's outputs), else min(count + 1,
 *   row_len).  Kernel launches only (a captured step holds no memset node); nothing is written outside hist and count. */
int ka_spectator_words(int which);
int ka_spectator_begin(int* count, int envs, void* stream);
int ka_spectator_note(const void* env_state, int state_bytes, int envs, const void* mask_bits, const long long* actions,
                      int action_mode, void* pending, void* stream);
int ka_spectator_commit(const void* err, const void* terminated, const void* truncated, int envs, const void* pending,
                        void* hist, int row_len, int* count, void* stream);

/* ---- policy insight (csrc/insight.hip; what the reference's showcase shows next to a board, showcase/runner.py:151-173,
 * showcase/heatmap.py:40-49, showcase/inference.py:95, plus entropy, rank and the number of legal moves).  One launch
 * after the sampler and before the env step, one workgroup per row, the spatial action space only (A = 81 * 139, action =
 * from-square * 139 + slot in the mover's perspective).
 * Inputs per row b: logits (B, A) fp32 or bf16 (logits_bf16 != 0); legal: packed rows, legal_words == ka_mask_words(A);
 *   actions (B) int64: the chosen action; vlogits (B, 3) fp32 or NULL; players (B) uint8: the mover's colour, or NULL;
 *   model_of (B) int32 with K as in ka_policy_sample_play, or NULL (every row seated); temperature > 0; top_k in 1..8.
 * p = softmax(logits / temperature) over the legal actions (the row maximum is subtracted first).  One record of
 * ka_policy_insight_words(0, top_k) = 8 + 2 top_k 32-bit words per row; ka_policy_insight_words(which, top_k) gives the
 * word offsets: 1 flags (bit 0 valid, bit 1 the mover's colour, bit 2 the chosen action is legal), 2 chosen action (int32;
 *   -1 / A for an action below / above the action space), 3 n_legal (int32), 4 chosen_rank (int32: the legal actions whose
 *   raw logit is strictly greater than the chosen action's; -1 where the chosen action is not legal), 5 chosen_probability
 *   (fp32: p[action], 0 where it is not legal), 6 entropy (fp32: -sum p ln p in nats, 0 ln 0 = 0), 7 win_probability (fp32:
 *   softmax(vlogits)[0], 0 without vlogits), 8 the top_k candidate actions (int32), 9 their probabilities (fp32); which 10 =
 *   floats of a heat row (132); -1 for any other which or a top_k outside 1..8.  Word 7 of the record is reserved (0).
 *   Candidates: the legal actions ordered by raw logit, descending, equal logits by lower action; unused entries are
 *   action -1, probability 0.  A legal logit that is -inf or NaN is never a candidate.
 * heat (B, 132) fp32, the chosen move's family (the legal moves with its USI prefix): for a board move (slot < 132)
 *   heat[s] = p[from * 139 + s]; for a drop (slot 132 + d) heat[sq] = p[sq * 139 + 132 + d], sq in 0..80, the rest 0;
 *   illegal members 0; all 0 where the chosen action is not legal.
 * A row whose model_of lies outside [0, K), or without a legal action, is invalid: record and heat row all zeros.
 * flags[0] |= NaN in a legal logit of a valid row.
 * Written: last (B, words): the row's record, every launch; heat; and, with hist != NULL, hist (B, row_len, words) at slot
 *   count[b] (int32, the env's spectator move count read BEFORE the env step) when 0 <= count[b] < row_len -- nothing
 *   otherwise, never past the row.  No commit launch: a refused step leaves the count alone (the slot is overwritten by
 *   the next ply), a finished game sets it to 0 in ka_spectator_commit; entries [0, count) are the moves of the game in
 *   progress.  Kernel launch only, caller-owned buffers, no workgroup waits for another. */
int ka_policy_insight_words(int which, int top_k);
int ka_policy_insight(const void* logits, int logits_bf16, const void* legal, int legal_words, const long long* actions,
                      const float* vlogits, const void* players, const int* model_of, int K, float temperature, int top_k,
                      void* last, float* heat, void* hist, int row_len, const int* count, int* flags, int B, int A, void* stream);

/* ---- sampling controls (csrc/sampling.hip; the reference's showcase plays at SAMPLING_TEMPERATURE = 0.5,
 * showcase/runner.py:52, :155-163; its rollouts and tournaments draw at temperature 1).  ka_policy_sample_ctl is
 * ka_policy_sample_play with a temperature, a top-k cut and an opening schedule per model.  logits, legal, legal_words,
 * seed_dev, model_of, K, actions, logp, nlegal, flags, B, A as in ka_policy_sample_play; one workgroup per row.
 * ctl: K rows of 4 32-bit words in device memory, row m for model m, read on every launch (a new table applies from the
 *   next ply of a captured graph; the same contract as the start pool's header):
 *     word 0 fp32 temperature   1 fp32 opening_temperature   2 int32 opening_plies   3 int32 top_k
 * plies / ply_stride: the u32 game ply of row b at plies + b * ply_stride (both multiples of 4); NULL = ply "infinite".
 *   The game ply is the u32 at byte 100 of the env's state row (kPlyByte of csrc/shogi_rules.h, the owner of the layout): the ply of the position to move in, 0 at the start of every
 *   game, restarted games included (owners pass state + 100 with stride ka_shogi_env_state_bytes()).  The ply_count output
 *   of the step is NOT it: for a finished game that holds the finished game's length.
 * A seated row (m = model_of[b] in [0, K)) with game ply p:
 *   T = p < opening_plies ? opening_temperature : temperature
 *   S = every legal action when top_k == 0 or n_legal <= top_k, else the top_k legal actions that come first by raw logit
 *       descending, equal logits by lower action (the candidate order of ka_policy_insight); 1 <= top_k <= 64
 *   T == 0: greedy, the first action of that order, probability 1
 *   T > 0:  q_j ~ exp((z_j - max_S z) * (1 / T)) over S; the draw is the inverse CDF over S in ascending action order at the
 *           play sampler's uniform (the same 64-bit mix of (*seed_dev, b), the same 24 bits); where rounding leaves
 *           target >= total, the last action of S
 *   logp[b] = log(clamp(q_action, FLT_EPSILON, 1 - FLT_EPSILON)); nlegal[b] counts every legal action, not |S|.
 * flags[0] |= a NaN logit, flags[1] |= a row without a legal action (action 0, log-prob 0); a row outside [0, K) gets its
 * first legal action and log-prob 0 -- all as in ka_policy_sample_play.
 * The neutral row (T == 1, top_k == 0) gives ka_policy_sample_play's actions and logp for the same inputs and seed, bit for
 * bit.  The table's contents cannot be checked on the host side of a launch: a row with top_k outside [0, 64] or a negative
 * or non-finite temperature is read as the neutral row (keisei_amd.training.sampling validates before upload).
 * Refused: null tensors, a packed mask width other than ka_mask_words(A), a row that does not fit 64 KB of LDS, K < 1,
 * ply_stride < 4 with plies, misaligned ctl / plies.  Kernel launch only, no workgroup waits for another. */
int ka_policy_sample_ctl(const void* logits, int logits_bf16, const void* legal, int legal_words, const long long* seed_dev,
                         const int* model_of, int K, const void* ctl, const void* plies, int ply_stride, long long* actions,
                         float* logp, int* nlegal, int* flags, int B, int A, void* stream);

/* ---- lookahead (csrc/lookahead.hip; the reference never searches).  A one-ply value lookahead inside the ply, between the
 * sampler and the env step, per model: fork the env rows into one child row per candidate move, step the children with
 * ka_shogi_env_step as it is, evaluate them with the grouped forward as it is, and play the candidate whose child is worst
 * for the side to move there.  Four stages on one stream, kernel launches only, caller-owned buffers, no workgroup waits for
 * another, nothing on the host in between:
 *   ka_lookahead_fork(...)                                   records, child rows
 *   ka_shogi_env_step(child_state, child_keys, child_checks, child_actions, N * width, max_ply, 1, 1, NULL, child_mask_bits,
 *                     child_err, ...)                        its own err, stats and output buffers, no pool
 *   ka_stem / tower / heads_eval_grouped                     over the child observations with child_model_of, in a workspace
 *                                                            of their own (the parent's logits stay where they are)
 *   ka_lookahead_choose(...)                                 q, the choice, actions[e] of the active envs
 * table: K rows of 4 32-bit words in device memory, row m for model m, read by every launch (a new table applies from the
 *   next ply of a captured graph):   word 0 int32 width   1 fp32 prior_weight   2 int32 skip_plies   3 int32 reply_width
 *   (0 = one ply; outside [0, 8] reads as 0; ka_lookahead_fork and ka_lookahead_choose ignore it).  A row with width outside [0, 8], a negative or non-finite prior_weight or a negative skip_plies reads as off (width 0);
 *   a width above the launch's `width` is cut to it.
 * Env e with m = model_of[e] is active when m lies in [0, K), the row's width is positive, its game ply (the u32 at byte
 *   100 of its state row; without state rows: "infinite") is >= skip_plies, and it has a candidate.
 * Candidates: the first `width` legal actions by raw logit descending, equal logits by lower action (the order of
 *   ka_policy_insight and ka_policy_sample_ctl); a legal logit that is -inf or NaN is never one.  prior_j = the candidate's
 *   softmax probability over ALL legal actions at temperature 1 (row maximum subtracted; a NaN logit weighs nothing).
 * q_j = the child's reward (for the mover) where the child step terminated or truncated the game, else P(L) - P(W) of
 *   softmax(child_vlogits_j): the child is seen by its side to move.  A non-finite value logit of a live child: q_j = -inf
 *   and err bit 0.  u_j = q_j + prior_weight * prior_j (q_j alone at weight 0); the choice is the first j of the greatest u.
 * Record of an env, ka_lookahead_words(0, width) = 4 + 3 width 32-bit words:
 *   0 flags (bit 0 active, bit 1 the choice differs from the sampler's action, bit 2 the chosen move ended the game as a win
 *   for the mover)   1 chosen slot   2 n_cand   3 chosen action (the sampler's for an inactive env)   4.. width candidate
 *   actions (int32, -1 = unused)   4 + width.. width priors (fp32)   4 + 2 width.. width q (fp32)
 * ka_lookahead_words(which, width): 0 record words, 1 table words per model (4), 2 stats words (4: positions searched,
 *   choices that differ from the sampler's, chosen moves that won the game, choices of the reply search that differ from
 *   the one-ply choice), 3 the maximum width (8), 4 the maximum reply width (8), 5 the most grandchildren of an env (64); -1
 *   otherwise.  A reply record has ka_lookahead_words(0, reply_width) words.
 * ka_lookahead_fork: logits (N, A) fp32 or bf16, legal packed rows (legal_words == ka_mask_words(A), A = 81 * 139), actions
 *   (N) int64 the sampler's, state (N, 128) / keys (N, max(max_ply, 1)) u64 / checks (N, max(max_ply, 1)) u8: the env's rows,
 *   only read.  Written: records (N, words); child rows c = e * width + j: child_state (the 128-byte row), child_keys /
 *   child_checks (entries [0, ply) of the env's rows, slots in use only; same row stride), child_mask_bits (the env's current
 *   packed mask row: the child step validates against it), child_actions (candidate j; the env's own sampled action for an
 *   unused or inactive slot, legal whenever the main step's is), child_model_of (m; -1 for an unused or inactive slot).
 *   The env rows and child rows may all be NULL: records only (candidates and priors).
 * ka_lookahead_choose: child_vlogits (N * width, 3), child_rewards, child_terminated / child_truncated (u8) as the child step
 *   and the forward wrote them; child_err: the child step's two 64-bit error words (or NULL) -- non-zero means the child
 *   step refused an action, which is a bug: err bit 1, and no action is replaced.  actions (N) int64 is overwritten for the
 *   active envs; stats (4 int32) is added to with atomics, err (1 int32) is ORed; the caller clears both.
 * Refused: null tensors, another action space or mask width, width outside [1, 8], K < 1, misaligned rows (state, history
 *   and mask rows are copied in 16-byte pieces).
 *
 * Reply search, for the models whose table row has reply_width = r > 0: three more stages between the children's forward and
 * the choice, and ka_lookahead_choose_replies in the place of ka_lookahead_choose:
 *   ka_lookahead_fork_replies(...)                           reply records, grandchild rows g = (e * width + j) * r + k
 *   ka_shogi_env_step / ka_stem / tower / heads_eval_grouped over the N * width * reply_width grandchild rows, with an err, stats,
 *                                                            output buffers and a workspace of their own
 *   ka_lookahead_choose_replies(...)                         v, the min per child, the choice, actions[e]
 * Replies of child j of an active env, where the child is live (neither terminated nor truncated): its first r legal actions
 *   of the child's post-step mask by the raw policy logit of the env's model on the child's observation (child_logits, as the
 *   children's forward wrote them), in the candidate order; their priors are recorded and not used; skip_plies plays no part.
 * v_jk, the grandchild's value for the root mover: 0 - reward of the grandchild step where the game ended there (the env's
 *   reward is for the reply's mover), else P(W) - P(L) of softmax(grand_vlogits); a non-finite value logit of a live
 *   grandchild: v_jk = -inf and err bit 0.  q_j = min_k v_jk, the first minimum; a done child keeps its reward, a live child
 *   without a reply candidate its one-ply q.  u_j and the choice as above.  The one-ply q of every candidate is computed as
 *   well (a non-finite value logit of a live child stays err bit 0): the one-ply choice is its arg-max of u, and env flag bit 3
 *   and stats word 3 say that the choice differs from it.  An env whose model has reply_width 0 gets the record, action and
 *   counters of ka_lookahead_choose, to the bit.
 * Reply record of a child, 4 + 3 reply_width words, the env record's layout: 0 flags (bit 0 the child has replies)   1 the slot
 *   of the first minimum   2 the number of replies   3 that reply's action (without replies: the lowest legal action of the
 *   child's mask)   4.. reply actions   4 + r.. priors   4 + 2 r.. v (fp32).
 * ka_lookahead_fork_replies: the child rows as the child step and forward left them, only read: child_logits (M, A) fp32 or
 *   bf16, child_mask_bits (the post-step masks), child_model_of, child_state / child_keys / child_checks, child_terminated /
 *   child_truncated (u8), M = N * width.  Written: reply_records (M, words) and the grandchild rows as ka_lookahead_fork writes
 *   child rows; an unused or inactive grandchild slot (a done child's row is a restarted game) gets the lowest legal action of
 *   the child's own post-step mask and model -1.
 * ka_lookahead_choose_replies: the arguments of ka_lookahead_choose, the reply records and the grandchild step's and
 *   forward's outputs (N * width * reply_width rows); grand_err as child_err: err bit 2, and on bit 1 or 2 no action is replaced. */
int ka_lookahead_words(int which, int width);
int ka_lookahead_fork(const void* logits, int logits_bf16, const void* legal, int legal_words, const long long* actions,
                      const int* model_of, int K, const void* table, const void* state, const void* keys, const void* checks,
                      int max_ply, int width, void* records, void* child_state, void* child_keys, void* child_checks,
                      void* child_mask_bits, long long* child_actions, int* child_model_of, int N, int A, void* stream);
int ka_lookahead_choose(void* records, int width, const void* table, const int* model_of, int K, const float* child_vlogits,
                        const float* child_rewards, const void* child_terminated, const void* child_truncated,
                        const void* child_err, long long* actions, int* stats, int* err, int N, void* stream);
int ka_lookahead_fork_replies(const void* child_logits, int logits_bf16, const void* child_mask_bits, int legal_words,
                              const int* child_model_of, int K, const void* table, const void* child_state,
                              const void* child_keys, const void* child_checks, const void* child_terminated,
                              const void* child_truncated, int max_ply, int reply_width, void* reply_records, void* grand_state,
                              void* grand_keys, void* grand_checks, void* grand_mask_bits, long long* grand_actions,
                              int* grand_model_of, int M, int A, void* stream);
int ka_lookahead_choose_replies(void* records, int width, void* reply_records, int reply_width, const void* table,
                                const int* model_of, int K, const float* child_vlogits, const float* child_rewards,
                                const void* child_terminated, const void* child_truncated, const void* child_err,
                                const float* grand_vlogits, const float* grand_rewards, const void* grand_terminated,
                                const void* grand_truncated, const void* grand_err, long long* actions, int* stats, int* err,
                                int N, void* stream);

/* ---- tree search (csrc/lookahead.hip): best-first minimax over `expansions` forks of `width` rows per env, in the place of
 * the lookahead in the ply.  Expansion 0 is the lookahead's fork of the env; every later expansion forks the leaf of the
 * current principal variation.  All node rows lie in one pool of expansions * N * width rows: node (t, j) of env e is row
 * (t * N + e) * width + j, local node t * width + j, and slice t is the N * width rows of expansion t.  Per ply, on one stream:
 *   ka_lookahead_fork(...)                                   expansion 0: record (0, e), the rows of slice 0
 *   ka_shogi_env_step, ka_stem / tower / heads_eval_grouped  over slice 0 (logits and value logits stay in the pool)
 *   ka_search_advance(t = 0)                                 leaf q, backup, the leaf to fork next
 *   for t = 1 .. expansions - 1:  ka_search_expand(t), step and forward over slice t, ka_search_advance(t)
 * table: the lookahead's K x 4 words with word 3 = expansions (1..16; outside reads as 1); words 0-2 as ka_lookahead_fork
 *   reads them.  An env is active as for ka_lookahead_fork.
 * q(t, j), for the player who moved into the node: the reward of its step where the game ended there, else P(L) - P(W) of
 *   softmax(value logits) (non-finite: -inf and err bit 0).  val(n) = q(n) for a node never forked or forked without a
 *   candidate, else 0 - max_k val(child k), the first maximum.  The principal leaf: from the first maximum of
 *   u_j = val(0, j) + prior_weight * prior_j at the root (val alone at weight 0) down the first-maximum children until a node
 *   is done or was forked without a candidate (the search of the env is finished: it is inactive from then on) or was never
 *   forked (the leaf).  Expansion t < expansions_m forks the leaf's first width_m legal actions by the node's own logits.
 *   Behind the last expansion: the first maximum of u at the root replaces actions[e]; flag bit 3 = it differs from the
 *   same arg-max over q(0, j); pv (N, expansions) int32 = the chosen action, then the first-maximum children's actions down
 *   to the first node never forked or done, padded with -1.
 * Records: (expansions, N, 4 + 3 width) words, the lookahead's layout; slot and action of record (t, e) are the first-maximum
 *   child of the node expansion t forked, the q words the leaf q.  Tree of an env, ka_search_words(1, ..) = E + 2 E width
 *   words: parent[E] (the local node expansion t forked, -1 = none), val[E * width] fp32, by[E * width] (the expansion that
 *   forked the node, -1 = never).
 * ka_search_words(which, width, expansions): 0 record words, 1 tree words per env, 2 stats words (5: positions searched,
 *   choices that differ from the sampler's, chosen moves that won, choices that differ from the one-ply choice, expansions
 *   run summed over the envs), 3 the maximum width (8), 4 the maximum expansions (16), 5 table words per model; else -1.
 * ka_search_expand: ka_lookahead_fork_replies over the pool, workgroup e reading row parent_row[e] (logits, post-step mask,
 *   state, history, model) and writing rows e * width + j of slice t, which the node_* pointers name (checked against the
 *   pool's).  active[e] = 0, a done parent or a parent_row outside [0, t * N * width) forks nothing: the rows get state and
 *   mask of row e * width of slice 0 (a stepped or restarted position), the lowest legal action of that mask, model -1 and no
 *   history, so the step over the slice is never refused by them.  Parents lie below slice t: nothing aliases.
 * ka_search_advance: one thread per env after the forward of expansion t.  step_err: (expansions, 2) 64-bit words, the error
 *   words of every slice's step; a non-zero word of slices 0..t is err bit 1, and then nothing is chosen and no action is
 *   replaced.  Writes parent_row / active for expansion t + 1 and, at t = expansions - 1, actions, flags and pv; stats is
 *   added to with atomics, err is ORed; the caller clears both. */
int ka_search_words(int which, int width, int expansions);
int ka_search_expand(const void* pool_logits, int logits_bf16, const void* pool_mask_bits, int legal_words,
                     const int* pool_model_of, int K, const void* table, const void* pool_state, const void* pool_keys,
                     const void* pool_checks, const void* pool_terminated, const void* pool_truncated, int max_ply, int width,
                     int t, const int* parent_row, const int* active, void* records, void* node_state, void* node_keys,
                     void* node_checks, void* node_mask_bits, long long* node_actions, int* node_model_of, int N, int A,
                     void* stream);
int ka_search_advance(void* records, void* tree, int width, int expansions, int t, const void* table, const int* model_of,
                      int K, const float* pool_vlogits, const float* pool_rewards, const void* pool_terminated,
                      const void* pool_truncated, const void* step_err, long long* actions, int* parent_row, int* active,
                      int* pv, int* stats, int* err, int N, void* stream);

/* ---- visit-count (PUCT) search (csrc/mcts.hip), in the place of the lookahead or the tree search in the ply.  The node
 * pool, its slices, the records and every stage that moves rows are the tree search's; the tree policy is new.  Per ply:
 *   ka_lookahead_fork, step and forward over slice 0, ka_mcts_advance(t = 0)
 *   for t = 1 .. simulations - 1:  ka_search_expand(t), step and forward over slice t, ka_mcts_advance(t)
 * table: K x 4 words, row m for model m: int32 width (0..8, 0 = off), fp32 c_puct (finite, >= 0), int32 skip_plies, int32
 *   simulations (1..64; a word outside reads as 1; a value above the launch's is cut to it).  Words 0-2 are read as
 *   ka_lookahead_fork reads them and an env is active by its rule.
 * Node (t, j) is candidate j of simulation t, local node t * width + j, pool row (t * N + e) * width + j.  Per node: N
 *   (int32 visits), S (fp32 value sum for the player who moved into the node), P (fp32, the prior the fork that created the
 *   node wrote: priors are used at every depth), by (the simulation that forked it, -1 = never).  Per simulation: parent,
 *   the local node it selected (-1: simulation 0, or it did not run).  The root holds no statistics.
 * q(t, j) is the tree search's leaf value (the step's reward where the game ended there, else P(L) - P(W) of the value
 *   head); a non-finite value logit of a live node is err bit 0 and its q is 0, in the record and in every sum.
 * Simulation 0 is the lookahead's fork: every child gets N = 1, S = q.
 * Selection of simulation t >= 1 (t < simulations_m), from the root: at a node with children k, Npar = sum_k N_k,
 *   s_k = S_k / N_k, plus c * P_k * sqrtf(Npar) / (1 + N_k) when c > 0, all fp32 in that written order; the first maximum
 *   is chosen (ties keep the lower slot) and written as slot and action of the record whose candidates the children are.
 *   A chosen child that is live and was never forked is the leaf: it forks into slice t through ka_search_expand
 *   (by = t).  A chosen child that is done, or was forked without a candidate, is a revisit: nothing forks (active = 0).
 * Backup of simulation t, after its forward: every new child gets N = 1, S = q_k; v = max_k q_k, the first maximum; the
 *   leaf gets N += 1, S += 0 - v, its parent N += 1, S += v, the signs alternating up to the root's child.  A revisit -- and
 *   a fork that found no candidate -- adds the node's own q to it instead, the signs alternating above it.  One thread adds,
 *   in simulation order.
 * Choice, in the last launch: the root candidate of most visits (ties keep the lower slot: the higher logit) replaces
 *   actions[e]; flag bit 3 = it differs from the arg-max of q(0, j).  pv (N, simulations) int32: the chosen action, then
 *   the most visited child at each level (ties the lower slot) down to the first node never forked or done, padded with
 *   -1.  root_visits (N, width) int32 and root_values (N, width) fp32 (S / N, 0 for an unused slot or an inactive env).
 * Tree of an env, ka_mcts_words(1, ..) = E + 4 E width words: parent[E], N[E * width], S[E * width], P[E * width],
 *   by[E * width].
 * ka_mcts_words(which, width, simulations): 0 record words, 1 tree words per env, 2 stats words (6: positions searched,
 *   choices that differ from the sampler's, chosen moves that won, choices that differ from the one-ply choice, simulations
 *   run and revisits, both summed over the envs), 3 the maximum width (8), 4 the maximum simulations (64), 5 table words per
 *   model, 7 the exploration's counter words (below); else -1.
 * ka_mcts_advance: one thread per env after the forward of simulation t, in this order: leaf q of slice t, backup,
 *   selection for t + 1 (parent_row / active for ka_search_expand), and at t = simulations - 1 the choice.  step_err:
 *   (simulations, 2) 64-bit words, the error words of every slice's step; a non-zero word of slices 0..t is err bit 1, and
 *   then nothing is selected, chosen or replaced.  stats is added to with atomics, err is ORed; the caller clears both. */
int ka_mcts_words(int which, int width, int simulations);
int ka_mcts_advance(void* records, void* tree, int width, int simulations, int t, const void* table, const int* model_of,
                    int K, const float* pool_vlogits, const float* pool_rewards, const void* pool_terminated,
                    const void* pool_truncated, const void* step_err, long long* actions, int* parent_row, int* active,
                    int* pv, int* root_visits, float* root_values, int* stats, int* err, int N, void* stream);

/* ---- exploration for the visit-count search (csrc/mcts_explore.hip, csrc/mcts_explore.h, the choice in csrc/mcts.hip):
 * Dirichlet noise mixed into the root priors, and for the first plies of a game the move drawn in proportion to the root
 * visits.  Per ply, with both on:
 *   ka_lookahead_fork, ka_mcts_root_noise, step and forward over slice 0, ka_mcts_advance_explore(t = 0), ...
 * explore_table: K rows of 4 32-bit words in device memory, row m for model m, read by every launch (a new table applies from
 *   the next ply of a captured graph):   0 fp32 noise_fraction epsilon in [0, 1]   1 fp32 noise_alpha in [0.01, 100] (not
 *   looked at when epsilon is 0)   2 int32 sample_plies in [0, 65535]   3 reserved, zero.  A row with a word out of range
 *   reads as off (all zero), and so does a model outside [0, K).
 * Random numbers: seed_dev points at the int64 the ply's sampler reads.  The stream of env e for purpose C is
 *   h = mix(seed ^ mix(e + C)) with mix = the splitmix64 finaliser behind every draw of the library, draw i of it
 *   r_i = mix(h + i * 0x9E3779B97F4A7C15), a uniform in (0, 1) is ((r >> 12) + 0.5) * 2^-52.  C = 0x2545F4914F6CDD1D for the
 *   noise and 0xD1342543DE82EF95 for the choice; the sampler's uniform uses 0x5851F42D4C957F2D.
 * ka_mcts_root_noise, behind ka_lookahead_fork and before ka_mcts_advance(t = 0): for every env whose record 0 has flag bit 0
 *   and whose model has epsilon > 0, with n = clamp(n_cand, 1, width): eta ~ Dirichlet(alpha) over the n candidates,
 *   s = p_0 + .. + p_{n-1} in slot order, p'_k = (1 - epsilon) p_k + epsilon s eta_k in fp64, rounded once to fp32 into the
 *   record's prior words (the prior mass of the candidates is kept).  Gamma(alpha) of slot k by Marsaglia-Tsang in fp64:
 *   a' = alpha < 1 ? alpha + 1 : alpha, d = a' - 1/3, c = 1 / sqrt(9 d); try j = 0..15 takes draws 64 k + 3 j + {0, 1, 2}:
 *   x = sqrt(-2 ln u0) cos(2 pi u1), v = (1 + c x)^3, rejected if v <= 0, accepted if ln u2 < 0.5 x^2 + d - d v + d ln v;
 *   g = d v, or d after 16 rejections; for alpha < 1 times exp(ln(u_b) / alpha), u_b draw 64 k + 48.  eta_k = g_k / sum g,
 *   the sum in slot order; 1 / n where the sum is not above 0 or not finite.  Written for a noised env only: the n prior words
 *   of the record, raw_priors (N, width) fp32 (the priors before, 0 in the unused slots) and eta (N, width) fp64 (0 in the
 *   unused slots); explore_stats[0] += the envs noised.  Nothing is written for any other env, and no slot >= n of a record.
 * ka_mcts_advance_explore: ka_mcts_advance (the same kernel; explore_table == NULL is ka_mcts_advance exactly, and the other
 *   four arguments are then not looked at).  With a table, behind the last simulation: best is the most visited root slot as
 *   before; p = the u32 at plies + e * ply_stride (the env's game ply: byte 100 of its state row).  Where p < sample_plies of
 *   the env's model the played slot is drawn: total = sum_{k<n} N_k, x = ((r_0 >> 32) * total) >> 32 on the choice stream,
 *   the first k whose running sum of N exceeds x (a slot without visits is never drawn); else it is best.  The played slot
 *   takes best's place in actions[e], slot and action of record 0, the changed / won bits and counters and the head of pv
 *   (the line beneath it: the most visited child at each level).  deepened, root_visits and root_values are unchanged.
 *   Record 0 flag bit 4 = the move was drawn, bit 5 = the drawn slot differs from best.
 * explore_stats, ka_mcts_words(7, ..) = 4 words (which = 6 stays unanswered, -1): envs noised, moves drawn, drawn moves that differ from best, reserved;
 *   added to with atomics, the caller clears them. */
int ka_mcts_root_noise(void* records, int width, const void* explore_table, const int* model_of, int K,
                       const long long* seed_dev, float* raw_priors, double* eta, int* explore_stats, int N, void* stream);
int ka_mcts_advance_explore(void* records, void* tree, int width, int simulations, int t, const void* table,
                            const int* model_of, int K, const float* pool_vlogits, const float* pool_rewards,
                            const void* pool_terminated, const void* pool_truncated, const void* step_err, long long* actions,
                            int* parent_row, int* active, int* pv, int* root_visits, float* root_values, int* stats, int* err,
                            const void* explore_table, const long long* seed_dev, const void* plies, int ply_stride,
                            int* explore_stats, int N, void* stream);

/* ---- mate in one (csrc/mate.hip; the reference never searches).  A rules-only mate check inside the ply, behind the
 * lookahead or the search and before the insight, per model: fork the env rows into one child row per checking move, step
 * the children with ka_shogi_env_step as it is, and play a child that ended by checkmate.  No forward runs.  Three stages on
 * one stream, kernel launches only, caller-owned buffers, no workgroup waits for another, nothing on the host in between:
 *   ka_mate_fork(...)                                        records, child rows
 *   ka_shogi_env_step(child_state, child_keys, child_checks, child_actions, N * cap, max_ply, 1, 1, NULL, child_mask_bits,
 *                     child_err, ...)                        its own err, stats and output buffers, no pool
 *   ka_mate_choose(...)                                      the mates, actions[e] of the envs that have one
 * table: K rows of 4 32-bit words in device memory, row m for model m, read by every launch (a new table applies from the
 *   next ply of a captured graph):   word 0 int32 max_checks (0 = off, 1..64)   1 int32 skip_plies (>= 0)   2, 3 reserved,
 *   zero.  A row with max_checks outside [0, 64] or a negative skip_plies reads as off; max_checks above the launch's `cap`
 *   is cut to it.
 * Env e with m = model_of[e] is active when m lies in [0, K), the row's max_checks is positive, its game ply (the u32 at
 *   byte 100 of its state row) is >= skip_plies, and it has a checking move.
 * Checking moves: the legal actions (the set bits of the env's packed mask row) after which the other king is attacked by
 *   the mover -- direct, discovered and double checks alike -- in ascending action order.  The first min(max_checks, cap)
 *   are forked.  A child is a mate when its slot is used, the child step set `terminated`, its termination reason is
 *   checkmate (1) and its reward is positive: the env step's verdict is the definition, so a checking move that ends the
 *   game by repetition, perpetual check or the move limit is not a mate.  If the incoming action is itself one of the
 *   mates it stays; otherwise the mate with the lowest action index replaces actions[e].
 * Record of an env, ka_mate_words(0, cap) = 4 + cap int32 words:
 *   0 flags (bit 0 active, bit 1 mate found, bit 2 the action was changed, bit 3 truncated: more checking moves than were
 *   forked)   1 checking moves, uncapped (0 for an env the controls leave out: its moves are not looked at)   2 the slot of
 *   the mate played, or -1   3 the action played (the incoming action unless bit 2)   4.. cap checking actions forked,
 *   ascending, -1 = unused
 * ka_mate_words(which, cap): 0 record words, 1 table words per model (4), 2 counter words (6: positions active, children
 *   forked, mates found, actions changed, positions truncated, then the error word), 3 the maximum cap (64); -1 otherwise.
 * ka_mate_fork: legal packed rows (legal_words == ka_mask_words(A), A = 81 * 139), actions (N) int64 the incoming actions,
 *   state (N, 128) / keys (N, max(max_ply, 1)) u64 / checks (N, max(max_ply, 1)) u8: the env's rows, only read.  Written:
 *   records (N, words); child rows c = e * cap + j: child_state (the 128-byte row), child_keys / child_checks (entries
 *   [0, ply) of the env's rows, slots in use only; same row stride), child_mask_bits (the env's current packed mask row: the
 *   child step validates against it), child_actions (checking move j; the env's own incoming action for an unused or
 *   inactive slot, legal whenever the main step's is -- nothing reads such a child's outcome).
 * ka_mate_choose: child_rewards, child_terminated (u8), child_reason (u8) as the child step wrote them; child_err: the child
 *   step's two 64-bit error words (or NULL) -- non-zero means the child step refused an action, which is a bug: err bit 1,
 *   and no action is replaced.  actions (N) int64 is overwritten where a mate replaces it; stats (5 int32) is added to with
 *   atomics, err (1 int32) is ORed; the caller clears both.
 * Refused: null tensors, another action space or mask width, cap outside [1, 64], K < 1, a misaligned table, misaligned rows
 *   (state, history and mask rows are copied in 16-byte pieces). */
int ka_mate_words(int which, int cap);
int ka_mate_fork(const void* legal, int legal_words, const long long* actions, const int* model_of, int K, const void* table,
                 const void* state, const void* keys, const void* checks, int max_ply, int cap, void* records,
                 void* child_state, void* child_keys, void* child_checks, void* child_mask_bits, long long* child_actions,
                 int N, int A, void* stream);
int ka_mate_choose(void* records, int cap, const float* child_rewards, const void* child_terminated, const void* child_reason,
                   const void* child_err, long long* actions, int* stats, int* err, int N, void* stream);

/* ---- mate in three (csrc/mate3.hip), behind the three stages of the mate in one and reusing them for the third ply.  On
 * the same stream, kernel launches only, caller-owned buffers, no workgroup waits for another:
 *   ka_mate_fork, ka_shogi_env_step, ka_mate_choose          the root, as above
 *   ka_mate3_fork(...)                                       the budget walk; the grandchild rows, one per evasion
 *   ka_shogi_env_step over the N * G grandchild rows         its own err, stats and output buffers
 *   ka_mate3_gate(...)                                       grand_model_of and a filler action per grandchild row
 *   ka_mate_fork, ka_shogi_env_step, ka_mate_choose          the third ply: the N * G grandchild rows as the envs, cap3 rows
 *                                                            each, grand_model_of, a second K x 4 table (word 0
 *                                                            reply_checks, word 1 zero), grand_filler as the action array
 *   ka_mate3_choose(...)                                     the proving set, actions[e], the record, the counters
 * table: the table of the mate in one; word 2 int32 evasion_rows (0 = mate in one only, 1..128), word 3 int32 reply_checks
 *   (0..64).  A row whose words 2 / 3 lie outside these ranges has depth three off, not its mate in one.
 * Env e is active at depth three when its mate-in-one record has bit 0 set and bit 1 clear and evasion_rows > 0.  Child i
 *   (root slot i) is open when its step neither terminated nor truncated it; n_i = the set bits of its new packed mask, the
 *   defender's evasions.  Budget walk in slot order, left = min(evasion_rows, G): an open child with 1 <= n_i <= left gets
 *   the next n_i grandchild rows of the env (one per evasion, ascending) and left -= n_i; an open child with n_i > left is
 *   skipped and the walk goes on.  A grandchild its step terminated or truncated refutes its check, whatever ended it and
 *   whatever the restarted row shows.  Child i proves when it got rows and every grandchild of it is open and its third-ply
 *   record has a mate.  A proving incoming action stays; otherwise the proving check with the lowest action replaces
 *   actions[e]; without one the action stands.
 * Record of an env, ka_mate3_words(0, cap) = 6 + 2 * cap int32 words:
 *   0 flags (bit 0 active at depth three, 1 mate in three found, 2 the action was changed, 3 a child was skipped by the
 *   budget, 4 a refuting grandchild's third-ply fork was truncated)   1 grandchild rows used   2 slot played, -1
 *   3 action played (the incoming action unless bit 2)   4, 5 the proving set as a 64-bit mask over the slots, low word
 *   first   6.. cap words n_i (-1: slot unused or not open)   6 + cap.. cap words first grandchild row of the slot within the
 *   env (-1: without rows)
 * ka_mate3_words(which, cap): 0 record words, 1 table words per model (4), 2 counter words (7: positions active at depth
 *   three, grandchild rows used, third-ply rows used, mates in three, actions changed, children skipped, then the error
 *   word), 3 the maximum G (128), 4 the maximum cap (64); -1 otherwise.
 * ka_mate3_fork: legal / actions / model_of / table / state as ka_mate_fork reads them (actions after ka_mate_choose);
 *   root_records and the child_* rows as the root's stages left them, child_mask_bits the child step's NEW masks; all only
 *   read.  Written: records (N, words); grandchild rows g = e * G + r: grand_state, grand_keys / grand_checks (entries
 *   [0, ply + 1) of the child's rows, rows in use only; same row stride), grand_mask_bits (the child's new mask: the step
 *   validates against it), grand_actions (the evasion; for an unused row the root env's state, mask and incoming action).
 * ka_mate3_gate: grand_mask_bits / grand_terminated / grand_truncated as the grandchild step wrote them.  Written:
 *   grand_model_of (N * G) int32 = model_of[e] for a used, open row, -1 otherwise; grand_filler (N * G) int64 = the first
 *   set bit of the row's new mask.
 * ka_mate3_choose: third_records (N * G, 4 + cap3) of the third ply; child_err / grand_err / third_err the two 64-bit error
 *   words of the three child steps: a non-zero one sets err bit 1 / 2 / 3 and nothing is replaced.  actions (N) int64 is
 *   overwritten where a mate in three replaces it; stats (6 int32) is added to with atomics, err (1 int32) is ORed; the
 *   caller clears both.
 * Refused: null tensors, another action space or mask width, cap outside [1, 64], G outside [1, 128], cap3 outside [1, 64],
 *   K < 1, misaligned rows. */
int ka_mate3_words(int which, int cap);
int ka_mate3_fork(const void* legal, int legal_words, const long long* actions, const int* model_of, int K, const void* table,
                  const void* state, const void* root_records, int cap, const void* child_state, const void* child_keys,
                  const void* child_checks, const void* child_mask_bits, const void* child_terminated,
                  const void* child_truncated, int max_ply, int G, void* records, void* grand_state, void* grand_keys,
                  void* grand_checks, void* grand_mask_bits, long long* grand_actions, int N, int A, void* stream);
int ka_mate3_gate(const void* records, int cap, int G, const int* model_of, const void* grand_mask_bits, int legal_words,
                  const void* grand_terminated, const void* grand_truncated, int* grand_model_of, long long* grand_filler,
                  int N, void* stream);
int ka_mate3_choose(void* records, const void* root_records, int cap, int G, const void* third_records, int cap3,
                    const void* grand_terminated, const void* grand_truncated, const int* model_of, int K,
                    const void* third_table, const void* child_err, const void* grand_err, const void* third_err,
                    long long* actions, int* stats, int* err, int N, void* stream);

/* ---- perft (csrc/perft.hip; the reference's is shogi-core's, game.rs:1206-1222).  The full-width fork: every legal move of
 * a frontier of positions becomes a complete env row, the rows are stepped by ka_shogi_env_step as it is, and counted.  The
 * host walks the tree depth-first over chunks (keisei_amd/perft.py); per chunk, on one stream, kernel launches only,
 * caller-owned buffers, no workgroup waits for another:
 *   ka_perft_plan(moves of level k, cursor, ...)             offset[p], header {taken, children, blocking row}; the host
 *                                                            reads the header
 *   ka_perft_fork(level k rows [cursor, cursor + taken))     the `children` rows of level k + 1
 *   ka_shogi_env_step(child_state, child_keys, child_checks, child_actions, children, max_ply, 1, 1, NULL,
 *                     child_mask_bits, ...)                  writes the children's new masks; its own err and outputs
 *   ka_perft_tally(level k + 1 rows [0, children))           moves of level k + 1, the counters
 * This is perft under the env's game rules: a row whose game ended has no successors -- the step has restarted it, so its
 * state and mask are a fresh game's, and moves[row] = 0 is what keeps it from being forked.
 * ka_perft_words(which): 0 counter columns per (tag, level) (4: nodes, ended by checkmate, ended otherwise, side to move in
 *   check), 1 header words (3), 2 the most moves a legal position has (593), 3 the largest cap (2^20), 4 the largest depth
 *   (8); -1 otherwise.
 * ka_perft_tally: n rows as a step left them -- state (n, 128), mask_bits (n, legal_words) the NEW packed masks, terminated /
 *   truncated / reason (n) u8 -- or, with the three NULL, rows nothing ended (the env's own).  tag (n) int32.  Written:
 *   moves[row] = 0 where terminated | truncated, else the set bits of the mask row below the action space.  With level in
 *   [0, depth): tally (tags, depth, 4) u64, row [tag][level] gets +1 node per row, +1 in column 1 where the row ended with
 *   reason checkmate (1), in column 2 where it ended otherwise, in column 3 where byte 96 of its state row (the side to move
 *   is in check; of the restarted game where the row ended) is set; level -1 counts none of these.  With leaf != 0:
 *   leaves[tag] (tags) u64 += moves[row].  Atomics, one per run of equal tags in a wave; the caller clears the tables.  A
 *   tag outside [0, tags) counts nowhere.
 * ka_perft_plan: one workgroup.  moves (n) int32, negative reads as 0.  taken = the largest t such that the moves of the
 *   parents [cursor, cursor + t) sum to at most cap; offset[p] = the sum of the moves of [cursor, p) for these parents
 *   (other entries are not written); header = {taken, children = their sum, s = cursor + taken if s < n and moves[s] > cap,
 *   else -1}.  A first parent with more than cap moves therefore gives taken = 0 and header[2] = cursor: the caller stops.
 * ka_perft_fork: one workgroup per parent p in [cursor, cursor + taken), of n parent rows: state / keys / checks as
 *   ka_mate_fork reads them, mask_bits the parents' current packed masks, moves / offset / tag (n) int32 as tally and plan
 *   left them.  A parent with moves[p] <= 0 forks nothing.  Otherwise child row c = offset[p] + r for the r-th set bit of
 *   the mask in ascending action order, r < moves[p]: child_state, child_keys / child_checks (entries [0, ply) of the
 *   parent's; same row stride), child_mask_bits (the parent's mask: the child step validates against it), child_actions[c]
 *   = the action, child_tag[c] = tag[p], or divide_base + c when divide_base >= 0 (the child's ordinal: perft_divide's
 *   first level).  err (1 int32) is ORed, the caller clears it: bit 0 the children of a parent would leave the cap rows
 *   (nothing of it is written), bit 1 a mask whose set bits are not moves[p] (no row outside offset[p] + [0, moves[p]) is
 *   written).
 * Refused: null tensors, another action space or mask width, cap outside [1, 2^20], parents outside [0, n), misaligned rows
 *   (state, history and mask rows are copied in 16-byte pieces), parent rows that overlap the child rows. */
int ka_perft_words(int which);
int ka_perft_tally(const void* state, const void* mask_bits, int legal_words, const void* terminated, const void* truncated,
                   const void* reason, const int* tag, int n, int level, int depth, int leaf, int tags, int* moves, void* tally,
                   void* leaves, void* stream);
int ka_perft_plan(const int* moves, int cursor, int n, int cap, int* offset, int* header, void* stream);
int ka_perft_fork(const void* state, const void* mask_bits, int legal_words, const void* keys, const void* checks,
                  const int* moves, const int* offset, const int* tag, int cursor, int taken, int n, int max_ply, int cap,
                  int divide_base, void* child_state, void* child_keys, void* child_checks, void* child_mask_bits,
                  long long* child_actions, int* child_tag, int* err, int A, void* stream);

/* ---- SL shard preparation (csrc/sl_prepare.hip; the replay keisei/sl/prepare.py:151-161 leaves out).  A batch of E game
 * records, game g in env g, stepped in lockstep from ka_shogi_env_reset.  One ply = ka_sl_replay_plan, ka_shogi_env_step
 * (unchanged), ka_sl_replay_record on one stream.
 * state: int32, ka_sl_replay_state_words(0) header words {0 plies, 1 records written, 2 filler steps, 3 games cut at an
 *   illegal move, 4 games the rules ended before the record did, 5 envs without a legal action, 6-7 copy of the VecEnv
 *   refusal latch int64}, then cursor[E], valid_len[E], reason[E] (0 none, 1 illegal move, 2 ended by the rules).  The host
 *   zeroes the header and the cursors and sets valid_len = the record's length before the first ply (the kernels
 *   take no length of their own).  which: 0 = header words, 1 = arrays
 *   of E words behind it, 2 = largest E, 3 = bytes of a shard record (16 220).
 * plan: the move actions[offset[g] + cursor] against the packed mask row of the position to move.  Live and legal:
 *   act = the move, write = 1.  Otherwise act = the lowest legal action (a filler: the env step refuses a batch with any
 *   illegal action), write = 0; a live game with an illegal move is cut there (valid_len = cursor, reason 1).
 * record: if write, shard row row_of[g] + cursor = {f32 obs[4050] of the position BEFORE the move (the env's previous
 *   buffer), i64 policy = act, i64 value 0 / 1 / 2 = W / D / L for the mover players[e] under outcome[g] (0 black wins,
 *   1 white wins, 2 draw), f32 score = material[e] / 76} in 4-byte stores (a row is 4-byte aligned only); rows outside
 *   [0, rows) are not written.  A game whose step reported terminated | truncated with moves left is cut (valid_len =
 *   cursor + 1, reason 2); the cursor advances. */
int ka_sl_replay_state_words(int which);
int ka_sl_replay_plan(int* state, int envs, const int* actions, int total, const int* offset, const void* mask_bits,
                      int mask_words, long long* act, int* write, void* stream);
int ka_sl_replay_record(int* state, int envs, const int* outcome, const int* row_of, const float* obs, int obs_elems,
                        const void* players, const long long* act, const int* write, const int* material,
                        const void* terminated, const void* truncated, const long long* refusal, void* shard, int rows,
                        void* stream);

/* ---- packed, device-resident SL dataset (csrc/sl_data.hip; keisei_amd/sl/device_dataset.py).  Every channel of a shard
 * record's observation is a 0/1 piece plane or a spatially constant plane, so a mask and one value per channel hold it bit
 * for bit.  Packed record = KA_SL_PACKED_WORDS dwords (816 bytes, rows 16-byte aligned):
 *   [3c, 3c+3)  c in 0..49: occupancy of channel c.  Bit p of the 96-bit little-endian field is set iff the 32-bit PATTERN
 *               of obs[c*81 + p] is non-zero (-0.0 is non-zero); bits 81..95 are zero.
 *   150 + c     the pattern shared by the non-zero squares of channel c; 0 when the mask is empty.
 *   200         policy as int32;  201 value as int32;  202 the score's bits;  203 zero.
 * A record is packable iff in every channel all non-zero patterns are equal; its targets are valid iff policy lies in
 * [0, 11259) and value in {0, 1, 2} (the score is not inspected).
 * pack: packed row i from the 16 220-byte record src_rows[i] (int64, device), or record i when src_rows is null; all loads
 *   are 4-byte loads (a record is 4-byte aligned only).  flags: int32[4] {unpackable records, lowest unpackable i, records
 *   with an invalid target, lowest such i}; the counts are added to, the indices taken as minima (the host sets them to
 *   INT_MAX).  A flagged record's packed row is written but is not a faithful copy: the caller raises.
 * gather: batch row b < B = packed row idx[b] (int64, device) decoded into obs_out[b] (fp32 NCHW (50, 9, 9), 8-byte
 *   aligned), policy_out[b] / value_out[b] (int64), score_out[b] (fp32).  An idx[b] outside [0, n) adds 1 to flags[0] and
 *   gives a row of zeros with targets 0; nothing outside the n packed rows is read. */
#define KA_SL_PACKED_WORDS 204
int ka_sl_packed_words(void);
int ka_sl_pack(const void* records, const long long* src_rows, int n, void* packed_out, int* flags, void* stream);
int ka_sl_gather(const void* packed, long long n, const long long* idx, int B, float* obs_out, long long* policy_out,
                 long long* value_out, float* score_out, int* flags, void* stream);
/* gather with the left-right reflection of the board (files reversed, ranks kept; shogi's rules are symmetric under it):
 *   mode 0  ka_sl_gather.
 *   mode 1  every row is reflected.
 *   mode 2  row b is reflected iff h >> 63, h = mix(seed ^ mix((((u64)epoch << 32) | (u32)i) + 0x6D6972726F72)), i = idx[b],
 *           mix = the splitmix64 finaliser (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *           x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31): a function of (seed, epoch, position) alone, whatever the
 *           batch, its order or the launch geometry.  epoch >= 0.
 * A reflected row is the plain row with obs[c][r][f] taken from obs[c][r][8 - f] (mask bit r * 9 + (8 - f) of the packed
 * record) and the policy target a = square * 139 + slot, if it lies in [0, 11259), replaced by mirror(a):
 *   square (r, f) -> (r, 8 - f);
 *   slot < 128 (promote = slot & 64, dir = (slot & 63) >> 3 clockwise from north, dist = slot & 7): dir -> (8 - dir) % 8;
 *   slot 128 + 2 * side + promote (knight): side -> 1 - side;   slots 132..138 (drops) unchanged.
 * mirror is an involution on [0, 11259); the white perspective (80 - q) commutes with it.  Value and score are unchanged.  An
 * idx[b] outside [0, n) gives a zero row with targets 0 and adds 1 to flags[0] in every mode. */
int ka_sl_gather_aug(const void* packed, long long n, const long long* idx, int B, float* obs_out, long long* policy_out,
                     long long* value_out, float* score_out, int* flags, int mode, long long seed, int epoch, void* stream);
/* Visit rows: a dataset may hold, beside every packed position, KA_SL_VISIT_WORDS visit words and KA_SL_INFO_WORDS info
 * words (for every position or for none).  Visit word k = action | visits << 16 (action < 11259, visits 0 = the slot is
 * unused); info = {model | mover << 16, index of the move in its game, env, game number}.
 * gather_visits: batch row b < B from visit row idx[b]: actions_out[b][k] (int32) = the action of a used slot, -1 of an
 * unused one; weights_out[b][k] (fp32) = (float)N_k / (float)(sum of the row's N), one IEEE division, 0 for an unused slot.
 * mode, seed, epoch as ka_sl_gather_aug: the rows it reflects have every used slot's action replaced by mirror(a), the
 * same draw of (seed, epoch, idx[b]).  An idx[b] outside [0, n) gives an all-unused row (the observation gather counts
 * it); flags (int32[1], may be null) counts the used words whose action lies outside [0, 11259), handed on as stored. */
#define KA_SL_VISIT_WORDS 8
#define KA_SL_INFO_WORDS 4
int ka_sl_gather_visits(const void* visits, long long n, const long long* idx, int B, int mode, long long seed, int epoch,
                        int* actions_out, float* weights_out, int* flags, void* stream);

/* ---- search samples (csrc/search_samples.hip; keisei_amd/training/search_samples.py): the positions a visit-count search
 * looked at, written as training rows inside the ply.  Per env a region of rows_per_env sample rows of
 * KA_SEARCH_SAMPLE_WORDS = 204 + 8 + 4 dwords (864 bytes): the packed position (above), the visit words, the info words.
 * Per-env meta, int32[5]: {write cursor, first row of the game in progress, samples dropped, moves played in the game in
 * progress, games finished}; the host zeroes it (and the error word) when the envs are reset.
 * step: one launch per ply, one workgroup per env, behind ka_shogi_env_step and before the loop's bookkeeping launch
 *   rewrites model_of.  obs_prev / players_prev are the env's PREVIOUS result buffers (the position before the move and
 *   its player to move, intact until the step after the next one); records (envs, rec_words) are the search's records of
 *   simulation 0 (word 0 bit 0 = active, word 2 = n_cand, words 4.. = the candidates' actions), root_visits (envs, width)
 *   the root candidates' visits, width <= 8; actions the actions stepped; material, rewards, terminated, truncated the
 *   step's results.
 * Write rule: a sample is written iff record 0 is active, n_cand >= 1 and model_of[e] >= 0.  The observation is packed as
 *   ka_sl_pack packs it; policy = actions[e] (the move played, after any mate override: not necessarily the most visited);
 *   value = -1 (unlabelled); score = the bits of (float)material[e] / 76.0f; word 203 = 0; visit word j = candidate j's
 *   action | visits << 16 for j < n_cand (0 where the visits are 0); info = {model_of[e] | mover << 16, moves, e, games}.
 *   A full region drops the sample and counts it in the meta; an observation that cannot be held packed ORs 1 into *err.
 *   The move counter (and, at a game's end, the game counter) advances for every env on every ply, written or not.
 * Label rule: where terminated | truncated, the winner is the game log's: the mover if rewards[e] > 0, the other side if
 *   < 0, nobody otherwise (a NaN included).  Every row of the region from the game's first row to the cursor, the new one
 *   included, gets value 0 where its mover is the winner, 2 where it is the loser, 1 for a draw; the game's first row moves
 *   to the cursor.
 * No env reads another env's words; the one atomic is the OR into *err.  which: 0 = words of a sample row, 1 = meta words
 * per env, 2 = visit words, 3 = info words, 4 = the largest number of envs. */
#define KA_SEARCH_SAMPLE_WORDS 216
int ka_search_sample_words(int which);
int ka_search_sample_step(const float* obs_prev, int obs_elems, const void* players_prev, const int* records, int rec_words,
                          const int* root_visits, int width, const int* model_of, const long long* actions,
                          const int* material, const float* rewards, const void* terminated, const void* truncated,
                          void* rows, int rows_per_env, int* meta, int* err, int envs, void* stream);

/* ---- transformer encoder path (BASELINE config 5; keisei/training/models/transformer.py:37-95: nn.Linear(50, d),
 * row/col nn.Embedding, nn.TransformerEncoder(nn.TransformerEncoderLayer(d, nhead, 4d, batch_first, norm_first), L),
 * nn.Linear(81 d, 11259), value head).  Tokens are (B*81, d) row-major, bf16 (autocast) or fp32 (parity mode; its linear
 * layers run on ka_gemm).  Dropout masks (nn.Dropout p = 0.1 inside the encoder layer, transformer.py:45-50) come from a
 * counter-based hash of (seed, element index): recomputed in the backward, never stored. */
/* C = epilogue(A * B^T), bf16 operands [M][lda] / [N][ldb] (K % 32 == 0), fp32 accumulate: forward nn.Linear (B = bf16
 * weight copy), its input gradient (B = transposed copy) and its weight gradient (A, B = transposed activations, nsplit
 * slabs over the token axis).  epilogue = +bias, ReLU, dropout, +residual, bf16 or fp32 store. */
int ka_tf_gemm_nt(const void* A, const void* B, void* C, const float* bias, const void* residual, int M, int N, int K,
                  int lda, int ldb, int ldc, int c_bf16, int relu, int nsplit, float drop_p, unsigned long long seed,
                  void* stream);
int ka_tf_gemm_nt_slabs(int K, int nsplit);
/* C (bf16) = (A B^T) * dropout_keep(seed, element) * [relu_act > 0]: the input-gradient GEMM of linear2 carrying the
 * backward of the dropout and ReLU that follow linear1 in the forward (transformer.py:45-50 via nn.TransformerEncoderLayer) */
int ka_tf_gemm_nt_masked(const void* A, const void* B, void* C, const void* relu_act, int M, int N, int K, int lda, int ldb,
                         int ldc, float drop_p, unsigned long long seed, void* stream);
/* dW = dY^T X straight from the row-major activations (weight gradient of nn.Linear, transformer.py:40-61): C[z][N][ldc]
 * fp32 slabs over token ranges (z < ka_tf_gemm_tn_slabs(M, nsplit); one slab = the result), A [M][lda] (N columns) and
 * B [M][ldb] (K columns) bf16, N / K / lda / ldb multiples of 8.  Operand fragments by LDS transpose reads: no transposed copies. */
int ka_tf_gemm_tn(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int nsplit, void* stream);
/* the same launch also producing the bias gradient of the layer: colsum [ka_tf_gemm_tn_slabs(M, nsplit)][N] = column sums of A
 * per token range (four more MFMAs per step against an all-ones fragment; db = sum of the slabs) */
int ka_tf_gemm_tn_bias(const void* A, const void* B, float* C, float* colsum, int M, int N, int K, int lda, int ldb, int ldc,
                       int nsplit, void* stream);
int ka_tf_gemm_tn_slabs(int M, int nsplit);
int ka_tf_transpose_pad(const void* in, void* out, int M, int N, int ldi, int ldo, int dtype, void* stream);
int ka_tf_cast_pad(const void* in, void* out, long long M, int N, int ldi, int ldo, int dtype, void* stream);
/* the bf16 operand copies of n nn.Linear weights (transformer.py:37-52: in_proj / out_proj / linear1 / linear2 of every encoder
 * layer, policy_fc) in one launch and from one read of each weight: table rows {W fp32 (N, K), out (N, ldo) bf16, outT (K, ldt) bf16,
 * N, K, ldo, ldt, first tile}, ldo % 8 == 0, ldt % 8 == 0; total_tiles = sum of ceil(ldt / 64) * ceil(ldo / 64).
 * Same values as ka_tf_cast_pad + ka_tf_transpose_pad per layer. */
int ka_tf_weights16_multi(const void* table, int n, int total_tiles, void* stream);
/* x[b,s,:] += row_embed[s/9] + col_embed[s%9] (transformer.py:84-87) and the embedding gradients (scratch: 65*81*d floats) */
int ka_tf_add_pos(void* x, const float* row_embed, const float* col_embed, int B, int d, int dtype, void* stream);
int ka_tf_pos_grad(const void* dx, float* scratch, float* drow, float* dcol, int B, int d, int dtype, void* stream);
/* nn.LayerNorm(d) (eps 1e-5) forward / backward; part: (ka_tf_layernorm_parts(M) + 1) * 2 * d floats; dx = LN'(dy) + dres */
int ka_tf_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, long long M,
                        int d, float eps, int dtype, void* stream);
int ka_tf_layernorm_parts(long long M);
/* launch counts per kernel form (K = 256 GEMM, big-tile GEMM, super-tile map on / off, LDS epilogue on / off, register /
   LDS attention forward) into a host array of n counts: tests check that a KA_TF_* switch changed the form */
int ka_tf_route_counts(long long* out, int n);
int ka_tf_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                        const void* dres, void* dx, float* part, float* dgamma, float* dbeta, long long M, int d, int dtype,
                        void* stream);
/* the same with a second output dx_drop = dx * dropout_keep(seed, element) (NULL: none): the gradient entering the sub-layer
 * below through its dropout, written in the same pass */
int ka_tf_layernorm_bwd_drop(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                             const void* dres, void* dx, void* dx_drop, float drop_p, unsigned long long seed, float* part,
                             float* dgamma, float* dbeta, long long M, int d, int dtype, void* stream);
/* out = in * keep [* (act > 0)] [+ res] */
int ka_tf_drop_apply(const void* g_in, const void* act, const void* res, void* g_out, long long n, float drop_p,
                     unsigned long long seed, int dtype, void* stream);
int ka_tf_colsum(const void* a, float* part, float* out, long long M, int N, int nsplit, int dtype, void* stream);
int ka_tf_mean_pool(const void* x, float* pooled, int B, int d, int dtype, void* stream);
int ka_tf_head_grad(const float* dpooled, const void* dflat, void* dx, int B, int d, int dtype, void* stream);
int ka_tf_tanh(float* v, long long n, void* stream);
int ka_tf_tanh_bwd(const float* dy, const float* y, float* dx, long long n, void* stream);
/* nn.MultiheadAttention(d, nhead, batch_first) core over the 81 squares: softmax(Q K^T / sqrt(dh)) V per (board, head) on
 * the matrix cores, dropout on the probabilities in training; qkv [B*81][3d] (in_proj output), out [B*81][d],
 * lse [B][H][81] for the backward.  dh <= 64. */
int ka_tf_attention_fwd(const void* qkv, void* out, float* lse, int B, int H, int dh, float drop_p, unsigned long long seed,
                        int dtype, void* stream);
int ka_tf_attention_bwd(const void* qkv, const void* dout, const float* lse, void* dqkv, int B, int H, int dh, float drop_p,
                        unsigned long long seed, int dtype, void* stream);
/* ... with the forward's output handed in: D[query] = rowsum(dout * out) makes dQ and dK / dV two independent launches on the
 * register-resident path (bf16, dh <= 32); other shapes fall through to ka_tf_attention_bwd */
int ka_tf_attention_bwd_o(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int H, int dh,
                          float drop_p, unsigned long long seed, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEISEI_AMD_H */
