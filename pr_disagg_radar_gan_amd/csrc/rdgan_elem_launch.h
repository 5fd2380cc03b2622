// Launchers of the step's elementwise / reduction kernels (rdgan_elem.hip.h) on raw pointers.  The three step functions and the
// op-level test entries (rdgan_op_softmax_tail ... rdgan_op_diff_combine) both launch through these, so a parity test runs the
// grid and the split the step runs: none of that arithmetic is written twice.  Included by rdgan_api.hip behind ew_blocks.
#pragma once

// ---- tails of the last generator conv: remaining tap sums, bias, Softmax(axis=1), check_numerics (the flag word is OR-ed) ----
// P[rows][32] of the plain column GEMM, one thread per (sample, h, w) column
static void launch_colgather_softmax(const float* P, const float* bias, float* out, int B, int H, int W, int* flag, hipStream_t st) {
  const long ncol = (long)B * H * W;
  hipLaunchKernelGGL(k_colgather_softmax, dim3((unsigned)((ncol + 63) / 64)), dim3(64), 0, st, P, bias, out, B, RDGAN_NHOURS, H, W, flag);
}
// Q[b][d][gq][h][w] with gq = 3 (9) in-tile tap sums per grid point; four lanes per column, 64 columns per workgroup
static void launch_tapsum_softmax_q(int gq, const float* Q, const float* bias, float* out, int B, int H, int W, int* flag, hipStream_t st) {
  const dim3 grid((unsigned)(((long)B * H * W + 63) / 64));
  if (gq == 3) hipLaunchKernelGGL((k_tapsum_softmax<RDGAN_NHOURS, 3>), grid, dim3(256), 0, st, Q, bias, out, B, H, W, flag);
  else hipLaunchKernelGGL((k_tapsum_softmax<RDGAN_NHOURS, 9>), grid, dim3(256), 0, st, Q, bias, out, B, H, W, flag);
}
// QT[b][item][tp][p][q][64] behind the slab kernel with the fused last conv (16 x 16 grid points); four columns per lane
static void launch_tapsum_softmax12(const float* Q12, const float* bias, float* out, int B, int* flag, hipStream_t st) {
  const long ncol = (long)B * 256;
  hipLaunchKernelGGL((k_tapsum_softmax12<RDGAN_NHOURS>), dim3((unsigned)((ncol / 4 + 63) / 64)), dim3(256), 0, st, Q12, bias, out, B, flag);
}
// dl = p * (g - sum_d p g), one thread per column
static void launch_softmax_bwd(const float* p, const float* g, float* dl, int B, int H, int W, hipStream_t st) {
  const long ncol = (long)B * H * W;
  hipLaunchKernelGGL(k_softmax_bwd, dim3((unsigned)((ncol + 63) / 64)), dim3(64), 0, st, p, g, dl, B, RDGAN_NHOURS, H, W);
}

// ---- gradient-penalty norm (X2): S workgroups per sample when there are few samples of many elements (ndomain 64) ----
static inline int gp_norm_slices(int B, int per) { return std::max(1, std::min({(1024 + B - 1) / B, per / 4096, 64})); }
// part: B * S floats (read and written only when S > 1)
static void launch_gp_norm(const float* g0, float* part, float* cin_hat, float* gpv, int per, int B, int CP, int S, hipStream_t st) {
  if (S > 1) hipLaunchKernelGGL(k_gp_norm_part, dim3(B * S), dim3(256), 0, st, g0, part, per, S);
  hipLaunchKernelGGL(k_gp_norm_r0, dim3(B * S), dim3(256), 0, st, g0, cin_hat, gpv, per, B, RD_GP_WEIGHT, CP, S, part);
}

// ---- loss tails (X3, T:408): out[0..7]; zero1 (critic, may be null) is cleared too ----
static void launch_critic_losses(const float* v, const float* gp, float* out8, int B, const int* gflag, float* zero1, hipStream_t st) {
  hipLaunchKernelGGL(k_critic_losses, dim3(1), dim3(256), 0, st, v, gp, out8, B, RD_GP_WEIGHT, gflag, zero1);
}
static void launch_gen_loss(const float* v, float* out8, int B, const int* gflag, hipStream_t st) {
  hipLaunchKernelGGL(k_gen_loss, dim3(1), dim3(256), 0, st, v, out8, B, gflag);
}

// ---- the critic's Dense layer (D6) and the top of its input-gradient chain; a16: h4 / u4 are bf16 ----
static void launch_critic_dense_fwd(bool a16, const void* h4, const float* w, const float* bias, float* v, int NB, int F, hipStream_t st) {
  if (a16) hipLaunchKernelGGL(k_critic_dense_fwd<rd_bf16_t>, dim3(NB), dim3(256), 0, st, (const rd_bf16_t*)h4, w, bias, v, F);
  else hipLaunchKernelGGL(k_critic_dense_fwd<float>, dim3(NB), dim3(256), 0, st, (const float*)h4, w, bias, v, F);
}
static void launch_critic_top_bwd(bool a16, const void* h4, const float* w, void* u4, int NB, int F, int B, int mode, uint64_t seed,
                                  hipStream_t st) {
  const int use_drop = seed != 0;
  const dim3 g(ew_blocks((long)NB * F));
  if (a16) hipLaunchKernelGGL(k_critic_top_bwd<rd_bf16_t>, g, dim3(256), 0, st, (const rd_bf16_t*)h4, w, (rd_bf16_t*)u4, NB, F, B, mode,
                              use_drop, rd_make_key(seed, RD_STREAM_D1 + 3));
  else hipLaunchKernelGGL(k_critic_top_bwd<float>, g, dim3(256), 0, st, (const float*)h4, w, (float*)u4, NB, F, B, mode, use_drop,
                          rd_make_key(seed, RD_STREAM_D1 + 3));
}
// row slices of the Dense weight gradient: the option's value, else one per 384 samples of the 3B batch; 16 at the most
static inline int dense_wgrad_slices(int forced, int NB) { return forced > 0 ? std::min(16, forced) : std::max(1, std::min(16, NB / 384)); }
// dW6 [F] into `out`; part: RS * F floats (used only when RS > 1)
static void launch_critic_dense_wgrad(bool a16, const void* buf, float* out, float* part, int NB, int F, int B, int RS, hipStream_t st) {
  float* dwo = RS > 1 ? part : out;
  const dim3 dg((F + 15) / 16, RS);
  if (a16) hipLaunchKernelGGL(k_critic_dense_wgrad<rd_bf16_t>, dg, dim3(256), 0, st, (const rd_bf16_t*)buf, dwo, NB, F, B);
  else hipLaunchKernelGGL(k_critic_dense_wgrad<float>, dg, dim3(256), 0, st, (const float*)buf, dwo, NB, F, B);
  if (RS > 1) hipLaunchKernelGGL(k_reduce_partials, dim3((F + 15) / 16), dim3(256), 0, st, part, RS, F, out);
}

// ---- hour differences of the shared-centre form and their adjoint; P = floats per hour plane (P % 4 == 0) ----
static void launch_diff_d(bool a16, const void* x, void* E, int B, int D, long P, hipStream_t st) {
  const dim3 dg(ew_blocks((long)B * (D + 1) * P / 4));
  if (a16) hipLaunchKernelGGL(k_diff_d<rd_bf16_t>, dg, dim3(256), 0, st, (const rd_bf16_t*)x, (rd_bf16_t*)E, B, D, P);
  else hipLaunchKernelGGL(k_diff_d<float>, dg, dim3(256), 0, st, (const float*)x, (float*)E, B, D, P);
}
static void launch_combine_dx(bool a16, void* dx, const void* dE, int B, int D, long P, hipStream_t st) {
  const dim3 cg(ew_blocks((long)B * D * P / 4));
  if (a16) hipLaunchKernelGGL(k_combine_dx<rd_bf16_t>, cg, dim3(256), 0, st, (rd_bf16_t*)dx, (const rd_bf16_t*)dE, B, D, P);
  else hipLaunchKernelGGL(k_combine_dx<float>, cg, dim3(256), 0, st, (float*)dx, (const float*)dE, B, D, P);
}

// ---- weight forms of a generator block (read only the weights) and their adjoints; cc = Cin * Cout (cc % 4 == 0) ----
// collapsed form Wc [64 = phase * 8 + tap][cc] and the fold of its gradient back onto the 27 taps
static void launch_collapse_weights(const float* W, float* Wc, long cc, hipStream_t st) {
  hipLaunchKernelGGL(k_collapse_weights, dim3(ew_blocks(16L * cc)), dim3(256), 0, st, W, Wc, (int)cc);
}
static void launch_fold_collapsed_wgrad(const float* dWc, float* dW, long cc, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_collapsed_wgrad, dim3(ew_blocks(27L * cc / 4)), dim3(256), 0, st, dWc, dW, (int)cc);
}
// shared-centre form U [48][cc] (the map: fastd_weight_map) and its adjoint
static void launch_weight_transform(const float* W, float* U, long cc, hipStream_t st) {
  RdWeightMap wm;
  fastd_weight_map(wm);
  hipLaunchKernelGGL(k_weight_transform, dim3(ew_blocks(48L * cc / 4)), dim3(256), 0, st, W, U, (int)cc, 48, wm);
}
static void launch_weight_transform_adj(const float* dU, float* dW, long cc, hipStream_t st) {
  RdWeightMap wm;
  fastd_weight_map(wm);
  hipLaunchKernelGGL(k_weight_transform_adj, dim3(ew_blocks(27L * cc / 4)), dim3(256), 0, st, dU, dW, (int)cc, 48, wm);
}

// ---- critic input (D0 + X1): the four-voxel kernel where the layout allows it ----
static inline bool critic_input_v4_ok(int nc, int CP, int HW, long total) { return nc == 1 && CP == 2 && HW % 4 == 0 && total < 0x7FFFFFFFL; }
static void launch_critic_input(const float* real, const float* fake, const float* cond, float* out, int B, int D, int HW, int nc, int CP,
                                int mode, uint32_t akey, uint32_t abase, bool v4, hipStream_t st) {
  const long total = (long)B * D * HW;
  if (v4) hipLaunchKernelGGL(k_build_critic_input_v4, dim3(ew_blocks(total / 4)), dim3(256), 0, st, real, fake, cond, out, B, D, HW, mode, akey, abase);
  else hipLaunchKernelGGL(k_build_critic_input, dim3(ew_blocks(total)), dim3(256), 0, st, real, fake, cond, out, B, D, HW, nc, CP, mode, akey, abase);
}

// ---- gradient wrt the generator's Dense pre-activation: LeakyReLU' from the stored output, with or without the pooling ----
// n4 = quads of elements; a16: g and h are bf16 (out is fp32)
static void launch_lrelu_bwd(bool a16, const void* g, const void* h, float* out, long n4, hipStream_t st) {
  const dim3 lg(ew_blocks(n4));
  if (a16) hipLaunchKernelGGL(k_lrelu_bwd<rd_bf16_t>, lg, dim3(256), 0, st, (const rd_bf16_t*)g, (const rd_bf16_t*)h, out, n4);
  else hipLaunchKernelGGL(k_lrelu_bwd<float>, lg, dim3(256), 0, st, (const float*)g, (const float*)h, out, n4);
}
// gup [B][2D][2H][2W][C], h0 and out [B][D][H][W][C]
static void launch_pool_lrelu_bwd(const float* gup, const float* h0, float* out, int B, int D, int H, int W, int C, hipStream_t st) {
  const long npix = (long)B * D * H * W;
  hipLaunchKernelGGL(k_pool_lrelu_bwd, dim3(ew_blocks(npix * (C / 4))), dim3(256), 0, st, gup, h0, out, npix, D, H, W, C);
}
