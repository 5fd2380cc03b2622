// Host side of librdgan_hip.so: plans, workspace, step orchestration and the C ABI of
// include/rdgan.h.  gfx950 only.  T = gan_train_cwgangp_pixelnorm.py,
// L = alternative_domains/gan_train_cwgangp_pixelnorm_largedomain.py in the reference.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include <algorithm>
#include <unordered_set>

#include "../../include/rdgan.h"
#include "rdgan_plan.h"
#include "rdgan_hostplan.h"
#include "rdgan_rng.h"
#include "rdgan_gemm.hip.h"
#include "rdgan_gemm_ws.hip.h"
#include "rdgan_gemm_ws16.hip.h"
#include "rdgan_gemm_f16.hip.h"
#include "rdgan_upconv16.hip.h"
#include "rdgan_upconv16b.hip.h"
#include "rdgan_upconv16t.hip.h"
#include "rdgan_elem.hip.h"
#include "rdgan_data.hip.h"
#include "rdgan_edge.hip.h"
#include "rdgan_d2slab16.hip.h"
#include "rdgan_d2fwd16.hip.h"
#include "rdgan_upwgrad16.hip.h"
#include "rdgan_upwgrad16b.hip.h"
#include "rdgan_d2wgrad16.hip.h"
#include "rdgan_d3wgrad16.hip.h"
#include "rdgan_d1fwd16.hip.h"
#include "rdgan_g9bwd16.hip.h"
#include "rdgan_spectral.hip.h"
#include "rdgan_rainfarm.hip.h"
#include "rdgan_crps.hip.h"
#include "rdgan_dist.hip.h"
#include "rdgan_radar.hip.h"
#include "rdgan_field.hip.h"
#include "rdgan_products.hip.h"
#include "rdgan_hourly.hip.h"        // what the evaluations of hourly arrays below share
#include "rdgan_verify.hip.h"
#include "rdgan_temporal.hip.h"
#include "rdgan_cells.hip.h"
#include "rdgan_sal.hip.h"
#include "rdgan_iss.hip.h"
#include "rdgan_distmap.hip.h"
#include "rdgan_storms.hip.h"
#include "rdgan_areal.hip.h"
#include "rdgan_catchment.hip.h"
#include "rdgan_spacetime.hip.h"
#include "rdgan_analog.hip.h"
#include "rdgan_mvscore.hip.h"
#include "rdgan_cascade.hip.h"
#include "rdgan_extremes.hip.h"
#include "rdgan_sequence.hip.h"
#include "rdgan_assign.hip.h"
#include "rdgan_reduce.hip.h"
#include "rdgan_mvrank.hip.h"
#include "rdgan_scaling.hip.h"
#include "rdgan_handle.h"           // struct rdgan_handle by concern; RD_CHECK / RD_TRY, side_fork / side_join, ensure_lds, the profiling scopes
#include "rdgan_slab_launch.h"      // one launcher per slab kernel of the bf16 storage mode

// ------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------
// algorithmic FLOPs of one pass over a plan: 2 * sum over phases of (rows * taps) * K per tap * N

template <int BM, int BN, int WM, int WN, int BK, bool PARTIAL, bool SHIFT, bool SRC16 = false, bool OUT16 = false>
static int launch_conv_cfg(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const float* src,
                           const float* W, int ldw, float* dst, const RdEpi& epi, hipStream_t st) {
  constexpr int AST = BK == 32 ? BK : BK + 4, BST = BN;
#ifdef RD_ONE_BLOCK_PER_CU
  constexpr size_t lds = 150 * 1024;      // diagnostic build: one workgroup per CU (no partner wave on a SIMD)
#else
  // the BK = 32 kernels reuse the staging LDS for the output tile + BM row bases in the epilogue
  constexpr size_t lds_loop = 2 * (size_t)(BM * AST + BK * BST) * sizeof(float);
  constexpr size_t lds_epi = BK == 32 ? ((size_t)BM * BN * sizeof(float) + (size_t)BM * 16) : 0;
  constexpr size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
#endif
  auto kern = k_conv_gemm<BM, BN, WM, WN, BK, PARTIAL, SHIFT, SRC16, OUT16>;
  RD_KNAME(h, "k_conv_gemm<%d,%d,BK%d>", BM, BN, BK);
  RD_TRY(ensure_lds(h, (const void*)kern, lds));
  long tm = plan_tiles(hp, B, BM);
  if (tm <= 0) return 0;
  {  // a tile's buffer descriptor is based at its first sample: its span must stay below 2 GiB
    long minL = hp.ph[0].L;
    for (int i = 1; i < hp.nphases; ++i) minL = std::min<long>(minL, hp.ph[i].L);
    if (std::min<long>(B, BM / minL + 2) * hp.src_sample * 4 >= 0x7FFFFFF0L) return bad_arg(h, "conv: source tile span exceeds 2 GiB");
    if (std::min<long>(B, BM / minL + 2) * hp.dst_sample * 4 >= 0x7FFFFFF0L) return bad_arg(h, "conv: destination tile span exceeds 2 GiB");
  }
  const long blocks = tm * (hp.N / BN);
  // split-K for small-M / large-K layers (critic tail, Dense, first generator block): few workgroups, long K loops
  RdEpi e2 = epi;
  e2.ksplit = 1; e2.kpart = nullptr; e2.kstride = 0;
  const long nch = (long)hp.ph[0].ntaps * ((hp.SC + BK - 1) / BK);
  const long total = (long)B * hp.dst_sample;
  if (epi.addt && BK != 32) return bad_arg(h, "conv: the shared-centre epilogue needs the BK = 32 kernels");
  if (h && !OUT16 && blocks < 256 && nch >= 16 && hp.d_cstride == hp.N && hp.N % 4 == 0 && epi.mode != RD_EPI_BIAS_PN_LRELU && !epi.addt) {
    long ks = std::min<long>(std::min<long>(8, 640 / blocks), nch / 4);
    for (int i = 1; i < hp.nphases; ++i) ks = std::min<long>(ks, (long)hp.ph[i].ntaps * ((hp.SC + BK - 1) / BK) / 2);
    if (ks >= 2 && (size_t)(ks * total) <= h->kpartial_cap) { e2.ksplit = (int)ks; e2.kpart = h->kpartial; e2.kstride = total; }
  }
  dim3 grid((unsigned)blocks, (unsigned)e2.ksplit);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, dp, B, src, W, ldw, dst, e2);
  if (e2.ksplit > 1)
    hipLaunchKernelGGL(k_splitk_finish<false>, dim3((unsigned)std::min<long>((total / 4 + 255) / 256, 2048)), dim3(256), 0, st, dst,
                       total, hp.N, e2);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

template <int BM, int BN, int WM, int WN, int TG, bool BF>
static int launch_conv_ws_tg(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const float* src,
                             const float* W, int ldw, float* dst, const RdEpi& epi, hipStream_t st, bool res = false);
// Resident-tile mode of the bf16 kernel (k_conv_gemm_ws<..., RES>): every phase's taps are (h,w)-shifted views of the same
// source planes (same d offset, offsets in [-1,1], unit stride, loop grid = source (h,w) grid), whole planes per tile, and
// the tile's rows for all channel chunks plus two weight stages fit the 80 KiB a workgroup may use at two per CU
static bool conv16_resident_ok(const RdPlan& hp, int BM, int BN) {
  if (hp.s_shift || hp.SC % 64) return false;
  const int plane = hp.SH * hp.SW;
  if (plane < 1 || plane > BM || BM % plane) return false;
  if ((size_t)(hp.SC / 64) * BM * 128 + 2 * (size_t)BN * 128 > 80 * 1024) return false;
  for (int i = 0; i < hp.nphases; ++i) {
    const RdPhase& q = hp.ph[i];
    if (q.ntaps < 1 || q.ntaps > 4 || q.LH != hp.SH || q.LW != hp.SW || q.L % plane) return false;
    for (int a = 0; a < 3; ++a) if (q.s_mul[a] != 1) return false;
    for (int t = 0; t < q.ntaps; ++t) {
      if (q.tap_off[t][0] != q.tap_off[0][0]) return false;
      if (q.tap_off[t][1] < -1 || q.tap_off[t][1] > 1 || q.tap_off[t][2] < -1 || q.tap_off[t][2] > 1) return false;
    }
  }
  return true;
}
// TG = taps whose gather offsets a loader wave keeps in registers: 4 when no phase has more (shared-centre plans).
// BF = bf16 operands (src / W point at bf16 data, W stored [tap block][N][K]); see k_conv_gemm_ws.
template <int BM, int BN, int WM, int WN, bool BF = false>
static int launch_conv_ws_cfg(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const float* src,
                              const float* W, int ldw, float* dst, const RdEpi& epi, hipStream_t st, bool res = false) {
  int maxtaps = 0;
  for (int i = 0; i < hp.nphases; ++i) maxtaps = std::max(maxtaps, hp.ph[i].ntaps);
  if (maxtaps <= 4) return launch_conv_ws_tg<BM, BN, WM, WN, 4, BF>(h, hp, dp, B, src, W, ldw, dst, epi, st, res);
  return launch_conv_ws_tg<BM, BN, WM, WN, 8, BF>(h, hp, dp, B, src, W, ldw, dst, epi, st);
}
template <int BM, int BN, int WM, int WN, int TG, bool BF>
static int launch_conv_ws_tg(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const float* src,
                             const float* W, int ldw, float* dst, const RdEpi& epi, hipStream_t st, bool res) {
  constexpr size_t lds_loop = 2 * (size_t)(BM * 32 + 32 * BN) * sizeof(float);
  constexpr size_t lds_epi = (size_t)BM * BN * sizeof(float) + (size_t)BM * 16;
  constexpr size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
  auto kern = k_conv_gemm_ws<BM, BN, WM, WN, TG, BF>;
  if constexpr (BM == 256 && BN == 64 && (TG == 4 || BF)) {     // the dominant launch runs under its own symbol (same code)
    if (epi.nametag == 1) kern = k_conv_gemm_ws<BM, BN, WM, WN, TG, BF, 1>;
    if constexpr (BF && TG == 4) {
      if (res) kern = epi.nametag == 1 ? k_conv_gemm_ws<BM, BN, WM, WN, TG, true, 1, true> : k_conv_gemm_ws<BM, BN, WM, WN, TG, true, 0, true>;
    } else res = false;
  } else res = false;
  if constexpr (!BF) {
    // "split3": the same launch on the bf16 matrix pipe from operands split three ways in registers (rdgan_gemm_ws.hip.h)
    if (h && h->split3) kern = k_conv_gemm_ws<BM, BN, WM, WN, TG, false, 0, false, true>;
  }
  RD_KNAME(h, "k_conv_gemm_ws<%d,%d,TG%d%s%s>", BM, BN, TG, BF ? ",bf16" : "", res ? ",res" : "");
  RD_TRY(ensure_lds(h, (const void*)kern, lds));
  constexpr int KCH = BF ? 64 : 32;                    // K elements per chunk
  if (BF && hp.SC % 64) return bad_arg(h, "conv: bf16 operands need a multiple of 64 channels per tap");
  // (the kernel decodes its tile with shifts: round 3's first bf16 Dense launch, 24 column tiles, computed 8 of them -- silently)
  if (hp.N % BN || ((hp.N / BN) & (hp.N / BN - 1))) return bad_arg(h, "conv: the producer/consumer kernel needs N / BN to be a power of two");
  long tm = plan_tiles(hp, B, BM);
  if (tm <= 0) return 0;
  long minL = hp.ph[0].L;
  for (int i = 1; i < hp.nphases; ++i) minL = std::min<long>(minL, hp.ph[i].L);
  if (std::min<long>(B, BM / minL + 2) * hp.src_sample * 4 >= 0x7FFFFFF0L) return bad_arg(h, "conv: source tile span exceeds 2 GiB");
  if (std::min<long>(B, BM / minL + 2) * hp.dst_sample * 4 >= 0x7FFFFFF0L) return bad_arg(h, "conv: destination tile span exceeds 2 GiB");
  RdEpi e2 = epi;
  e2.ksplit = 1; e2.kpart = nullptr; e2.kstride = 0;
  const long blocks = tm * (hp.N / BN);
  // Wave quantisation: a mid-size launch of long workgroups (say 384 on 256 CUs) leaves a third of the chip idle in
  // its last round.  Split K so that the workgroup count fills whole rounds; the partial sums cost one extra pass over
  // the (small) output, priced at 3 % per split.
  const long total = (long)B * hp.dst_sample;
  if (h && h->ws_ksplit && !res && blocks < 1024 && hp.d_cstride == hp.N && epi.mode != RD_EPI_BIAS_PN_LRELU && !epi.addt) {
    long nch = (long)hp.ph[0].ntaps * (hp.SC / KCH);
    for (int i = 1; i < hp.nphases; ++i) nch = std::min<long>(nch, (long)hp.ph[i].ntaps * (hp.SC / KCH));
    auto cost = [&](long ks) { double r = (double)(blocks * ks) / 256.0; return std::ceil(r) / r * (1.0 + 0.03 * (ks - 1)); };
    long best = 1;
    for (long ks = 2; ks <= 8; ++ks)
      if (nch / ks >= 12 && (size_t)(ks * total) <= h->kpartial_cap && cost(ks) < cost(best) - 0.02) best = ks;
    if (h->ws_ksplit > 1) best = std::min<long>(h->ws_ksplit, std::max<long>(1, nch / 4));   // tests: force a split
    if (best > 1 && (size_t)(best * total) <= h->kpartial_cap) { e2.ksplit = (int)best; e2.kpart = h->kpartial; e2.kstride = total; }
  }
  if (!BF) e2.out16 = 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)e2.ksplit), dim3(512), lds, st, dp, B, src, W, ldw, dst, e2);
  if (e2.ksplit > 1) {
    const dim3 fg((unsigned)std::min<long>((total / 4 + 255) / 256, 2048));
    if (e2.out16) hipLaunchKernelGGL(k_splitk_finish<true>, fg, dim3(256), 0, st, dst, total, hp.N, e2);
    else hipLaunchKernelGGL(k_splitk_finish<false>, fg, dim3(256), 0, st, dst, total, hp.N, e2);
  }
  RD_CHECK(h, hipGetLastError());
  return 0;
}

static int launch_conv(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const float* src, const float* W,
                       int ldw, float* dst, const RdEpi& epi, hipStream_t st, int tag) {
  ProfScope ps(h, tag, st);
  LaunchScope ls(h, plan_index(h, hp), RD_KIND_CONV, B, plan_flops(hp, B), st);
  if (h) h->flops_acc += plan_flops(hp, B);
  const bool partial = (hp.SC & 3) != 0, shift = hp.s_shift != 0;
  if (partial && shift) return bad_arg(h, "conv: SC % 4 != 0 with a folded upsample is not supported");
  if (hp.SC < 32 && hp.SC != 27) {   // small-K taps (D1): BK = 8
    if (hp.N % 64 || shift) return bad_arg(h, "conv: unsupported BK=8 case");
    if (partial) return launch_conv_cfg<128, 64, 2, 2, 8, true, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
    return launch_conv_cfg<128, 64, 2, 2, 8, false, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
  }
#define RD_CONV(BM_, BN_, WM_, WN_)                                                                                  \
  do {                                                                                                               \
    if (partial) return launch_conv_cfg<BM_, BN_, WM_, WN_, 32, true, false>(h, hp, dp, B, src, W, ldw, dst, epi, st); \
    if (shift) return launch_conv_cfg<BM_, BN_, WM_, WN_, 32, false, true>(h, hp, dp, B, src, W, ldw, dst, epi, st);   \
    return launch_conv_cfg<BM_, BN_, WM_, WN_, 32, false, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);             \
  } while (0)
  const bool ws_ok = h && h->wave_spec && !partial && !shift && hp.SC % 32 == 0;
  if (ws_ok && h->wave_spec == 2) {      // test mode: the producer/consumer kernel regardless of the problem size
    if (hp.N % 128 == 0) return launch_conv_ws_cfg<128, 128, 2, 2>(h, hp, dp, B, src, W, ldw, dst, epi, st);
    if (hp.N == 64) return launch_conv_ws_cfg<256, 64, 4, 1>(h, hp, dp, B, src, W, ldw, dst, epi, st);
  }
  // at most 64 rows (the generator's Dense layer at ndomain 64 with 64 samples: 64 x 4196 against 4196 x 49152 weights): a
  // 128-row tile would multiply 64 rows of zeros -- the launch streams its 825 MB of weights at 1.5 TB/s, the 64-row tile at 2.6
  if (hp.nphases == 1 && (long)B * hp.ph[0].L <= 64 && hp.N % 64 == 0 && !shift) RD_CONV(64, 64, 2, 2);
  // phases of unequal length (stride-2 input gradients: 8 ... 1 taps): the 8-tap workgroups set the launch time, so a
  // mid-size launch takes the narrower tile (twice the workgroups, half the work each)
  int tmin = hp.ph[0].ntaps, tmax = tmin;
  for (int i = 1; i < hp.nphases; ++i) { tmin = std::min(tmin, hp.ph[i].ntaps); tmax = std::max(tmax, hp.ph[i].ntaps); }
  const bool uneven = tmax >= 2 * tmin;
  if (hp.N % 128 == 0 && plan_tiles(hp, B, 128) * (hp.N / 128) >= 200 &&
      !(uneven && ws_ok && plan_tiles(hp, B, 128) * (hp.N / 128) < 1024)) {
    if (ws_ok) return launch_conv_ws_cfg<128, 128, 2, 2>(h, hp, dp, B, src, W, ldw, dst, epi, st);
    RD_CONV(128, 128, 2, 2);
  }
  if (hp.N % 64 == 0) {
    // N = 64 layers with plenty of rows: 256-row tile so every wave owns a 64x64 tile (64 MFMAs per barrier)
    if (hp.N == 64 && !shift && plan_tiles(hp, B, 256) >= 1024) {   // (the SHIFT variant of this tile would spill)
      if (ws_ok) return launch_conv_ws_cfg<256, 64, 4, 1>(h, hp, dp, B, src, W, ldw, dst, epi, st);
      if (partial) return launch_conv_cfg<256, 64, 4, 1, 32, true, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
      return launch_conv_cfg<256, 64, 4, 1, 32, false, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
    }
    if (plan_tiles(hp, B, 128) * (hp.N / 64) >= 200) {
      if (ws_ok) return launch_conv_ws_cfg<128, 64, 2, 2>(h, hp, dp, B, src, W, ldw, dst, epi, st);
      RD_CONV(128, 64, 2, 2);
    }
    // few rows, very long K (input gradient of the first generator block): producer/consumer kernel with its K split
    if (ws_ok && h->ws_ksplit && (hp.nphases == 1 || hp.boxes) && hp.d_cstride == hp.N && (long)hp.ph[0].ntaps * (hp.SC / 32) >= 96 &&
        plan_tiles(hp, B, 128) * (hp.N / 64) >= 32)
      return launch_conv_ws_cfg<128, 64, 2, 2>(h, hp, dp, B, src, W, ldw, dst, epi, st);
    RD_CONV(64, 64, 2, 2);
  }
  if (hp.N == 32 && !partial && !shift && epi.mode == RD_EPI_TAPGATHER)
    return launch_conv_cfg<256, 32, 4, 1, 32, false, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
  if (hp.N == 32 && !partial && !shift)
    return launch_conv_cfg<128, 32, 4, 1, 32, false, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
#undef RD_CONV
  return bad_arg(h, "conv: unsupported N");
}

// bf16 storage mode: the few GEMMs that stay on the fp32 matrix pipe (the generator's Dense layer and the first critic
// layer read fp32 inputs and write bf16; the 64 -> 1 conv reads bf16 and writes its fp32 tap sums)
static int launch_conv_a16(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const float* src, const float* W,
                           int ldw, float* dst, const RdEpi& epi, hipStream_t st, int tag, bool src16, bool out16) {
  ProfScope ps(h, tag, st);
  LaunchScope ls(h, plan_index(h, hp), RD_KIND_CONV, B, plan_flops(hp, B), st);
  if (h) h->flops_acc += plan_flops(hp, B);
  const bool partial = (hp.SC & 3) != 0;
  if (hp.s_shift) return bad_arg(h, "conv (bf16 storage): folded upsample is not supported");
  if (!src16 && out16) {
    if (hp.SC < 32 && hp.SC != 27) {      // first critic layer: BK = 8
      if (hp.N % 64) return bad_arg(h, "conv (bf16 storage): unsupported BK=8 case");
      if (partial) return launch_conv_cfg<128, 64, 2, 2, 8, true, false, false, true>(h, hp, dp, B, src, W, ldw, dst, epi, st);
      return launch_conv_cfg<128, 64, 2, 2, 8, false, false, false, true>(h, hp, dp, B, src, W, ldw, dst, epi, st);
    }
    if (!partial && hp.N % 64 == 0)        // Dense
      return launch_conv_cfg<64, 64, 2, 2, 32, false, false, false, true>(h, hp, dp, B, src, W, ldw, dst, epi, st);
  }
  if (src16 && !out16 && hp.N == 32 && !partial) {     // last generator conv as a column GEMM
    if (epi.mode == RD_EPI_TAPGATHER) return launch_conv_cfg<256, 32, 4, 1, 32, false, false, true, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
    return launch_conv_cfg<128, 32, 4, 1, 32, false, false, true, false>(h, hp, dp, B, src, W, ldw, dst, epi, st);
  }
  return bad_arg(h, "conv (bf16 storage): unsupported fp32-pipe GEMM");
}

static inline int ew_blocks(long n, int per = 256);
#include "rdgan_elem_launch.h"   // launchers of the elementwise kernels on raw pointers: shared with the op entries
// critic input (k_build_critic_input): the four-voxel kernel where the layout allows it
static void launch_build_critic_input(rdgan_handle* h, const float* real, const float* fake, const float* cond, int B, int mode,
                                      uint32_t akey, uint32_t abase, hipStream_t st) {
  const int D = h->ddim[0][0], HW = h->nd * h->nd;
  const long total = (long)B * D * HW;
  launch_critic_input(real, fake, cond, h->cin, B, D, HW, h->nc, h->CP, mode, akey, abase, critic_input_v4_ok(h->nc, h->CP, HW, total), st);
}
static inline int ew_blocks(long n, int per) { return (int)std::min<long>((n + per - 1) / per, 8192); }

// k_conv_gemm_f16 (rdgan_gemm_f16.hip.h): when a launch may take it
static bool conv_f16_ok(const rdgan_handle* h, const RdPlan& hp, int B, const RdEpi& epi) {
  if (h && !h->conv_f16) return false;
  if (hp.s_shift || hp.SC % 64 || hp.N % 128 || ((hp.N / 128) & (hp.N / 128 - 1)) || hp.w_rows_per_tap != hp.SC) return false;
  if (!epi.out16 || epi.addt) return false;
  if (epi.mode == RD_EPI_BIAS_PN_LRELU ? hp.N != 128 : epi.mode > RD_EPI_GATE_AUX) return false;
  for (int i = 0; i < hp.nphases; ++i) if (hp.ph[i].ntaps > 64) return false;
  // 256-row tiles, 512 resident at a time: below ~640 workgroups the streaming kernel (half the tile, its own K split) was the
  // faster one on every launch measured (scratch/f16_ab.py); conv_f16 = 2 (tests): regardless
  return (h && h->conv_f16 == 2) || !h || plan_tiles(hp, B, RD_F16_BM) * (hp.N / 128) >= 640;
}
static int launch_conv_f16(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const void* src16, const void* wfrag, float* dst,
                           const RdEpi& epi, hipStream_t st) {
  const bool pn = epi.mode == RD_EPI_BIAS_PN_LRELU;
  auto kern = pn ? k_conv_gemm_f16<true> : k_conv_gemm_f16<false>;
  int maxtaps = 0;
  for (int i = 0; i < hp.nphases; ++i) maxtaps = std::max(maxtaps, hp.ph[i].ntaps);
  const int tg = maxtaps <= 4 ? 4 : 8;                 // (the streaming kernel's tap groups: same chunk order, same sums)
  RD_KNAME(h, "k_conv_gemm_f16<256,128,bf16%s>", pn ? ",+pn" : "");
  RD_TRY(ensure_lds(h, (const void*)kern, RD_F16_LDS));
  long tm = plan_tiles(hp, B, RD_F16_BM);
  if (tm <= 0) return 0;
  long minL = hp.ph[0].L;
  for (int i = 1; i < hp.nphases; ++i) minL = std::min<long>(minL, hp.ph[i].L);
  if (std::min<long>(B, RD_F16_BM / minL + 2) * hp.src_sample * 4 >= 0x7FFFFFF0L) return bad_arg(h, "conv: source tile span exceeds 2 GiB");
  if (std::min<long>(B, RD_F16_BM / minL + 2) * hp.dst_sample * 4 >= 0x7FFFFFF0L) return bad_arg(h, "conv: destination tile span exceeds 2 GiB");
  RdEpi e2 = epi;
  e2.ksplit = 1; e2.kpart = nullptr; e2.kstride = 0;
  const long blocks = tm * (hp.N / 128);
  const long total = (long)B * hp.dst_sample;
  if (h && h->ws_ksplit > 1 && !pn && hp.d_cstride == hp.N) {        // tests: force a split
    long nch = (long)hp.ph[0].ntaps * (hp.SC / 64);
    for (int i = 1; i < hp.nphases; ++i) nch = std::min<long>(nch, (long)hp.ph[i].ntaps * (hp.SC / 64));
    const long best = std::min<long>(h->ws_ksplit, std::max<long>(1, nch / 4));
    if (best > 1 && (size_t)(best * total) <= h->kpartial_cap) { e2.ksplit = (int)best; e2.kpart = h->kpartial; e2.kstride = total; }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)e2.ksplit), dim3(256), RD_F16_LDS, st, dp, B, (const rd_bf16_t*)src16,
                     (const rd_bf16_t*)wfrag, (rd_bf16_t*)dst, e2, tg);
  if (e2.ksplit > 1)
    hipLaunchKernelGGL(k_splitk_finish<true>, dim3((unsigned)std::min<long>((total / 4 + 255) / 256, 2048)), dim3(256), 0, st, dst, total, hp.N, e2);
  RD_CHECK(h, hipGetLastError());
  return 0;
}
// [T][N][K] bf16 -> fragment order (the twin image k_conv_gemm_f16 reads)
static int launch_wfrag_image(rdgan_handle* h, const void* in, void* out, long T, int N, int K, hipStream_t st) {
  hipLaunchKernelGGL(k_wfrag_image, dim3((unsigned)std::min<long>((T * N * K / 8 + 255) / 256, 2048)), dim3(256), 0, st,
                     (const unsigned short*)in, (unsigned short*)out, T, N, K);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// bf16-operand conv GEMM (fp32 accumulate / output): src16 = bf16 NDHWC activations, w16 = bf16 weights [tap block][N][K];
// wfrag = the same weights in fragment order, or nullptr
static int launch_conv16(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const void* src16, const void* w16,
                         float* dst, const RdEpi& epi, hipStream_t st, int tag, const void* wfrag = nullptr) {
  ProfScope ps(h, tag, st);
  LaunchScope ls(h, plan_index(h, hp), RD_KIND_CONV, B, plan_flops(hp, B), st);
  if (h) h->flops_acc += plan_flops(hp, B);
  if (hp.s_shift || hp.SC % 64 || hp.N % 64) return bad_arg(h, "conv16: needs SC % 64 == 0, N % 64 == 0, no folded upsample");
  if (wfrag && conv_f16_ok(h, hp, B, epi)) return launch_conv_f16(h, hp, dp, B, src16, wfrag, dst, epi, st);
  const float* s = (const float*)src16; const float* w = (const float*)w16;
  if (hp.N % 128 == 0) return launch_conv_ws_cfg<128, 128, 2, 2, true>(h, hp, dp, B, s, w, 0, dst, epi, st);
  if (hp.N == 64 && plan_tiles(hp, B, 256) >= 512) {
    const bool res = (!h || h->resident) && conv16_resident_ok(hp, 256, 64);
    return launch_conv_ws_cfg<256, 64, 4, 1, true>(h, hp, dp, B, s, w, 0, dst, epi, st, res);
  }
  return launch_conv_ws_cfg<128, 64, 2, 2, true>(h, hp, dp, B, s, w, 0, dst, epi, st);
}
// fp32 -> bf16 copies (round to nearest even) of an activation tensor and of a weight-form stack [T][K][N] -> [T][N][K]
static int launch_to_bf16(rdgan_handle* h, const float* in, void* out, long n, hipStream_t st) {
  hipLaunchKernelGGL(k_to_bf16, dim3(ew_blocks(n / 8)), dim3(256), 0, st, in, (unsigned short*)out, n);
  RD_CHECK(h, hipGetLastError());
  return 0;
}
static int launch_weights_to_bf16_t(rdgan_handle* h, const float* in, void* out, int T, int K, int N, hipStream_t st, void* outf = nullptr) {
  hipLaunchKernelGGL(k_weights_to_bf16_t, dim3((N + 31) / 32, (K + 31) / 32, T), dim3(256), 0, st, in, (unsigned short*)out, K, N,
                     (unsigned short*)outf);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// true when launch_conv will pick a tile whose BN equals the plan's N, i.e. a workgroup owns whole output rows
static bool conv_rows_owned(const RdPlan& hp, int B) {
  if (hp.s_shift || (hp.SC & 3) || hp.SC < 32) return false;
  if (hp.N == 128) return plan_tiles(hp, B, 128) >= 200;
  if (hp.N == 64) return plan_tiles(hp, B, 256) >= 1024 || plan_tiles(hp, B, 128) >= 200;
  return false;
}

// the same for launch_conv16 (bf16 storage mode): tiles 128x128 (N % 128 == 0), 256x64 / 128x64 (N == 64)
static bool conv16_rows_owned(const RdPlan& hp) { return hp.N == 128 || hp.N == 64; }


template <int BR, int BN, bool PARTIAL, bool SHIFT, bool DY16 = false>
static int launch_wgrad_cfg(rdgan_handle* h, const RdPlan* dp, int nphases, int B, const float* src, const float* dy,
                            float* partial, const RdWgradTiling& T, int nsplit, hipStream_t st) {
  constexpr size_t lds = 2 * (size_t)(32 * BR + 32 * BN) * sizeof(float);
  auto kern = k_wgrad_gemm<BR, BN, PARTIAL, SHIFT, DY16>;
  RD_KNAME(h, "k_wgrad_gemm<%d,%d>", BR, BN);
  RD_TRY(ensure_lds(h, (const void*)kern, lds));
  dim3 grid((unsigned)(T.RT * T.NT * nsplit * nphases));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, dp, B, src, dy, partial, T);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

template <int BR, int BN>
static int launch_wgrad_ws_cfg(rdgan_handle* h, const RdPlan* dp, int nphases, int B, const float* src, const float* dy,
                               float* partial, const RdWgradTiling& T, int nsplit, hipStream_t st) {
  constexpr size_t lds_loop = 2 * (size_t)(32 * BR + 32 * BN) * sizeof(float);
  constexpr size_t lds_epi = (size_t)BR * BN * sizeof(float);
  constexpr size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
  auto kern = k_wgrad_gemm_ws<BR, BN>;
  RD_KNAME(h, "k_wgrad_gemm_ws<%d,%d>", BR, BN);
  RD_TRY(ensure_lds(h, (const void*)kern, lds));
  dim3 grid((unsigned)(T.box ? T.nsplit : T.RT * T.NT * nsplit * nphases));
  hipLaunchKernelGGL(kern, grid, dim3(512), lds, st, dp, B, src, dy, partial, T);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// dW (rows tap_w*wrpt + c, leading dimension ldw = N) from src (gathered through the plan) and dy
static int launch_wgrad(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const float* src, const float* dy,
                        float* dW, float* partial_ws, size_t partial_cap, hipStream_t st, int tag, bool dy16 = false) {
  ProfScope ps(h, tag, st);
  LaunchScope ls(h, plan_index(h, hp), RD_KIND_WGRAD, B, plan_flops(hp, B), st);
  if (h) h->flops_acc += plan_flops(hp, B);
  if (hp.N % 64) return bad_arg(h, "wgrad: N % 64 != 0");
  if (!hp.boxes)
  for (int i = 1; i < hp.nphases; ++i)
    if (hp.ph[i].ntaps != hp.ph[0].ntaps || hp.ph[i].L != hp.ph[0].L) return bad_arg(h, "wgrad: phases must be congruent");
  int BR, BN, nsplit;
  RdWgradTiling T = wgrad_tiling(hp, B, BR, BN, nsplit);
  size_t need = T.box ? (size_t)T.RT * BR * hp.N : (size_t)hp.nphases * nsplit * T.RT * BR * hp.N;
  if (T.box && !(h && h->wave_spec && (hp.SC & 3) == 0 && !hp.s_shift && !dy16))
    return bad_arg(h, "wgrad: border-class boxes only through k_wgrad_gemm_ws");
  if (need > partial_cap) return bad_arg(h, "wgrad: partial workspace too small");
  long minL = hp.ph[0].L;
  for (int i = 1; i < hp.nphases; ++i) minL = std::min<long>(minL, hp.ph[i].L);
  if (std::min<long>(B, T.rows_per_split / minL + 2) * std::max(hp.src_sample, hp.dst_sample) * 4 >= 0x7FFFFFF0L)
    return bad_arg(h, "wgrad: split span exceeds 2 GiB");
  const int np = hp.nphases;
  const bool partial = (hp.SC & 3) != 0, shift = hp.s_shift != 0;
  if (partial && (shift || BR != 64 || BN != 64)) return bad_arg(h, "wgrad: SC % 4 != 0 only with the 64x64 tile");
#define RD_WG(BR_, BN_)                                                                                           \
  do {                                                                                                            \
    if (shift) RD_TRY((launch_wgrad_cfg<BR_, BN_, false, true>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st))); \
    else RD_TRY((launch_wgrad_cfg<BR_, BN_, false, false>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));      \
  } while (0)
  float* partial_buf = partial_ws;
  const long wrows = (long)B * hp.ph[0].L;
  const bool ws = h && h->wave_spec && !partial && !shift && !dy16 && (h->wave_spec == 2 || wrows * hp.nphases >= 1024 || T.box);
  // one phase in one split through k_wgrad_gemm: the tiles go straight to dW, no partial slab, no fold (the Dense layer's 64-row K
  // loop at ndomain 64: the slab was 825 MB written, read and written again)
  const bool direct = !ws && !T.box && !dy16 && !partial && np == 1 && nsplit == 1 && h != nullptr && hp.ph[0].w_off == 0;
  if (direct) { T.direct = 1; T.ldw = hp.N; partial_buf = dW; }
  if (dy16) {       // bf16 storage mode, first critic layer: fp32 gathered input against the bf16 output gradient
    if (shift || BR != 64 || BN != 64) return bad_arg(h, "wgrad: bf16 output gradient only with the 64x64 tile");
    if (partial) RD_TRY((launch_wgrad_cfg<64, 64, true, false, true>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
    else RD_TRY((launch_wgrad_cfg<64, 64, false, false, true>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
  }
  else if (ws && BR == 256) RD_TRY((launch_wgrad_ws_cfg<256, 64>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
  else if (ws && BR == 128 && BN == 128) RD_TRY((launch_wgrad_ws_cfg<128, 128>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
  else if (ws && BR == 128) RD_TRY((launch_wgrad_ws_cfg<128, 64>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
  else if (ws && BN == 128) RD_TRY((launch_wgrad_ws_cfg<64, 128>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
  else if (ws) RD_TRY((launch_wgrad_ws_cfg<64, 64>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
  else if (partial) RD_TRY((launch_wgrad_cfg<64, 64, true, false>(h, dp, np, B, src, dy, partial_buf, T, nsplit, st)));
  else if (BR == 256) RD_WG(256, 64);
  else if (BR == 128 && BN == 128) RD_WG(128, 128);
  else if (BR == 128) RD_WG(128, 64);
  else if (BN == 128) RD_WG(64, 128);
  else RD_WG(64, 64);
#undef RD_WG
  if (direct) { RD_CHECK(h, hipGetLastError()); return 0; }
  if (T.box) {      // per weight tap: the slabs of every phase that lists it
    const int nw = 64 - __builtin_clzll(hp.wmask | 1ull);
    const long nout = (long)nw * hp.SC * (hp.N / 4);
    hipLaunchKernelGGL(k_wgrad_reduce_box, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, dp, partial_ws, T, BR, B, nw, dW, hp.N);
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  long total = (long)T.RT * BR * (hp.N / 4);
  int outs = 256;                       // output float4s per workgroup; the other 256/outs thread slices split the fold
  while (outs > 16 && (total + outs - 1) / outs * np < 512 && 256 / outs < nsplit) outs >>= 1;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((total + outs - 1) / outs), np), dim3(256), 0, st, dp, partial_ws,
                     nsplit, T, BR, dW, hp.N, outs);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// bf16-operand weight gradient (mixed mode): src16 / dy16 = bf16 copies of the gathered tensor and of the output gradient;
// same tiling, partial slabs and fold as launch_wgrad.  Tiles 256x64, 128x128, 128x64.
template <int BR, int BN>
static int launch_wgrad16_cfg(rdgan_handle* h, const RdPlan* dp, int nphases, int B, const void* src16, const void* dy16,
                              float* partial, const RdWgradTiling& T, int nsplit, hipStream_t st) {
  constexpr size_t lds_loop = ((BR == 256 && BN == 128) ? 3 : 2) * (size_t)(64 * BR * 2 + 64 * BN * 2);
  constexpr size_t lds_epi = (size_t)BR * BN * sizeof(float);
  constexpr size_t lds = lds_loop > lds_epi ? lds_loop : lds_epi;
  auto kern = k_wgrad_gemm_ws16<BR, BN>;
  RD_KNAME(h, "k_wgrad_gemm_ws16<%d,%d>", BR, BN);
  RD_TRY(ensure_lds(h, (const void*)kern, lds));
  dim3 grid((unsigned)(T.box ? T.nsplit : T.RT * T.NT * nsplit * nphases));
  hipLaunchKernelGGL(kern, grid, dim3(512), lds, st, dp, B, (const unsigned short*)src16, (const unsigned short*)dy16, partial, T);
  RD_CHECK(h, hipGetLastError());
  return 0;
}
static bool wgrad16_ok(const RdPlan& hp, int B) {
  int BR, BN, nsplit;
  if (hp.s_shift || hp.SC % 64 || hp.N % 64) return false;
  wgrad_tiling(hp, B, BR, BN, nsplit);
  return BR >= 128;
}
static bool wgrad16_wide(const rdgan_handle* h) { return !h || h->wgrad_wide; }     // (op-level entries: on, so that the tile stays tested)
static int launch_wgrad16(rdgan_handle* h, const RdPlan& hp, const RdPlan* dp, int B, const void* src16, const void* dy16,
                          float* dW, float* partial_ws, size_t partial_cap, hipStream_t st, int tag) {
  ProfScope ps(h, tag, st);
  LaunchScope ls(h, plan_index(h, hp), RD_KIND_WGRAD, B, plan_flops(hp, B), st);
  if (h) h->flops_acc += plan_flops(hp, B);
  if (!wgrad16_ok(hp, B)) return bad_arg(h, "wgrad16: needs SC % 64 == 0, N % 64 == 0, a 128- or 256-row tile, no folded upsample");
  if (!hp.boxes)
  for (int i = 1; i < hp.nphases; ++i)
    if (hp.ph[i].ntaps != hp.ph[0].ntaps || hp.ph[i].L != hp.ph[0].L) return bad_arg(h, "wgrad: phases must be congruent");
  int BR, BN, nsplit;
  RdWgradTiling T = wgrad_tiling(hp, B, BR, BN, nsplit, wgrad16_wide(h));
  size_t need = T.box ? (size_t)T.RT * BR * hp.N : (size_t)hp.nphases * nsplit * T.RT * BR * hp.N;
  if (need > partial_cap) return bad_arg(h, "wgrad: partial workspace too small");
  long minL16 = hp.ph[0].L;
  for (int i = 1; i < hp.nphases; ++i) minL16 = std::min<long>(minL16, hp.ph[i].L);
  if (std::min<long>(B, T.rows_per_split / minL16 + 2) * std::max(hp.src_sample, hp.dst_sample) * 2 >= 0x7FFFFFF0L)
    return bad_arg(h, "wgrad: split span exceeds 2 GiB");
  const int np = hp.nphases;
  if (BR == 256 && BN == 128) RD_TRY((launch_wgrad16_cfg<256, 128>(h, dp, np, B, src16, dy16, partial_ws, T, nsplit, st)));
  else if (BR == 256) RD_TRY((launch_wgrad16_cfg<256, 64>(h, dp, np, B, src16, dy16, partial_ws, T, nsplit, st)));
  else if (BN == 128) RD_TRY((launch_wgrad16_cfg<128, 128>(h, dp, np, B, src16, dy16, partial_ws, T, nsplit, st)));
  else RD_TRY((launch_wgrad16_cfg<128, 64>(h, dp, np, B, src16, dy16, partial_ws, T, nsplit, st)));
  if (T.box) {      // per weight tap: the slabs of every phase that lists it
    const int nw = 64 - __builtin_clzll(hp.wmask | 1ull);
    const long nout = (long)nw * hp.SC * (hp.N / 4);
    hipLaunchKernelGGL(k_wgrad_reduce_box, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, dp, partial_ws, T, BR, B, nw, dW, hp.N);
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  long total = (long)T.RT * BR * (hp.N / 4);
  int outs = 256;
  while (outs > 16 && (total + outs - 1) / outs * np < 512 && 256 / outs < nsplit) outs >>= 1;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((total + outs - 1) / outs), np), dim3(256), 0, st, dp, partial_ws,
                     nsplit, T, BR, dW, hp.N, outs);
  RD_CHECK(h, hipGetLastError());
  return 0;
}


// out[c] = sum over rows of src[rows][C]
static int launch_colsum(rdgan_handle* h, const float* src, long rows, int C, float* out, hipStream_t st, bool src16 = false) {
  ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
  const bool any = C != 64 && C != 128 && C != 256;
  if (src16 && any) return bad_arg(h, "colsum: bf16 input only for 64 / 128 / 256 columns");
  // (round 4 tried at most 256 partial rows with 1024-thread workgroups so that the fold is one round trip: beside the GEMMs of the
  // main stream such a workgroup waits for sixteen free wave slots on one CU -- block 3's sums went 62 -> 120-250 us; the fold got
  // small workgroups instead: k_reduce_partials4)
  long nblk = std::min<long>(1024, std::max<long>(1, rows / (any ? 8 : 32)));
  if ((size_t)nblk * C > h->cpartial_cap) nblk = std::max<long>(1, (long)(h->cpartial_cap / C));
  long rpb = (rows + nblk - 1) / nblk;
  nblk = (rows + rpb - 1) / rpb;
  dim3 grid((unsigned)nblk);
  const rd_bf16_t* s16 = (const rd_bf16_t*)src;
  const bool big = false;
#define RD_COLSUM(CG_, T_, P_)                                                                                                    \
  do {                                                                                                                            \
    if (big) hipLaunchKernelGGL((k_colsum_partial<CG_, T_, 1024>), grid, dim3(1024), 0, st, P_, rows, h->cpartial, rpb);          \
    else hipLaunchKernelGGL((k_colsum_partial<CG_, T_, 256>), grid, dim3(256), 0, st, P_, rows, h->cpartial, rpb);                \
  } while (0)
  if (src16 && C == 64) RD_COLSUM(16, rd_bf16_t, s16);
  else if (src16 && C == 128) RD_COLSUM(32, rd_bf16_t, s16);
  else if (src16) RD_COLSUM(64, rd_bf16_t, s16);
  else if (C == 64) RD_COLSUM(16, float, src);
  else if (C == 128) RD_COLSUM(32, float, src);
  else if (C == 256) RD_COLSUM(64, float, src);
#undef RD_COLSUM
  else {
    const int bt = std::max(64, std::min(256, (C + 63) / 64 * 64));
    hipLaunchKernelGGL(k_colsum_partial_any, dim3((unsigned)nblk, (C + bt - 1) / bt), dim3(bt), 0, st, src, rows, C, h->cpartial, rpb);
  }
  if (!any && nblk <= 1024)
    hipLaunchKernelGGL(k_reduce_partials4, dim3(C / 4), dim3(256), 0, st, h->cpartial, (int)nblk, C, out);
  else
  hipLaunchKernelGGL(k_reduce_partials, dim3((C + 15) / 16), dim3(rd_reduce_threads((int)nblk)), 0, st, h->cpartial, (int)nblk, C, out);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

static int launch_transpose(rdgan_handle* h, const float* in, float* out, int T, int R, int C, int ldo, hipStream_t st) {
  dim3 grid((C + 31) / 32, (std::max(R, ldo) + 31) / 32, T);
  hipLaunchKernelGGL(k_transpose, grid, dim3(256), 0, st, in, out, R, C, ldo);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

static int launch_pn_fwd(rdgan_handle* h, const float* y, float* hout, float* rinv, long npix, int C, hipStream_t st, bool a16 = false) {
  long threads = npix * (C / 4);
  dim3 grid((unsigned)((threads + 255) / 256));
  const rd_bf16_t* y16 = (const rd_bf16_t*)y; rd_bf16_t* h16 = (rd_bf16_t*)hout;
  if (a16) {
    if (C == 256) hipLaunchKernelGGL((k_pixelnorm_lrelu_fwd<64, rd_bf16_t>), grid, dim3(256), 0, st, y16, h16, rinv, npix);
    else if (C == 128) hipLaunchKernelGGL((k_pixelnorm_lrelu_fwd<32, rd_bf16_t>), grid, dim3(256), 0, st, y16, h16, rinv, npix);
    else if (C == 64) hipLaunchKernelGGL((k_pixelnorm_lrelu_fwd<16, rd_bf16_t>), grid, dim3(256), 0, st, y16, h16, rinv, npix);
    else return bad_arg(h, "pixelnorm: C must be 64/128/256");
  }
  else if (C == 256) hipLaunchKernelGGL(k_pixelnorm_lrelu_fwd<64>, grid, dim3(256), 0, st, y, hout, rinv, npix);
  else if (C == 128) hipLaunchKernelGGL(k_pixelnorm_lrelu_fwd<32>, grid, dim3(256), 0, st, y, hout, rinv, npix);
  else if (C == 64) hipLaunchKernelGGL(k_pixelnorm_lrelu_fwd<16>, grid, dim3(256), 0, st, y, hout, rinv, npix);
  else return bad_arg(h, "pixelnorm: C must be 64/128/256");
  RD_CHECK(h, hipGetLastError());
  return 0;
}
// dE (fp32 storage, pool = 0): the difference part's gradient [B][D + 1][H][W][C] that the kernel folds into g (k_combine_dx fused in)
static int launch_pn_bwd(rdgan_handle* h, const float* g, const float* hh, const float* rinv, float* dy, long npix, int C,
                         int pool, int D, int H, int W, hipStream_t st, bool a16 = false, const float* dE = nullptr) {
  long threads = npix * (C / 4);
  dim3 grid((unsigned)((threads + 255) / 256));
  if (dE && (a16 || pool || D < 1 || H < 1 || W < 1)) return bad_arg(h, "pixelnorm bwd: dE needs fp32 storage and the collapsed form");
#define RD_PNB(LP, PO) hipLaunchKernelGGL((k_pn_lrelu_bwd<LP, PO>), grid, dim3(256), 0, st, g, hh, rinv, dy, npix, D, H, W, dE)
#define RD_PNB16(LP) hipLaunchKernelGGL((k_pn_lrelu_bwd<LP, 0, rd_bf16_t>), grid, dim3(256), 0, st, (const rd_bf16_t*)g, \
                                        (const rd_bf16_t*)hh, rinv, (rd_bf16_t*)dy, npix, D, H, W, (const rd_bf16_t*)nullptr)
  if (a16) {
    if (pool) return bad_arg(h, "pixelnorm bwd: the bf16 storage mode needs the collapsed form");
    if (C == 256) RD_PNB16(64); else if (C == 128) RD_PNB16(32); else if (C == 64) RD_PNB16(16);
    else return bad_arg(h, "pixelnorm bwd: C must be 64/128/256");
  }
  else if (C == 256) { if (pool) RD_PNB(64, 1); else RD_PNB(64, 0); }
  else if (C == 128) { if (pool) RD_PNB(32, 1); else RD_PNB(32, 0); }
  else if (C == 64) { if (pool) RD_PNB(16, 1); else RD_PNB(16, 0); }
  else return bad_arg(h, "pixelnorm bwd: C must be 64/128/256");
#undef RD_PNB
#undef RD_PNB16
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// PixelNorm+LeakyReLU backward over hour-plane pairs, also writing the pair sums gS (shared-centre backward)
// dE (fp32 storage): the difference part's gradient [B][2 Ds + 1][HW][C], folded into g as in launch_pn_bwd
static int launch_pn_bwd_pairs(rdgan_handle* h, const float* g, const float* hh, const float* rinv, float* dy, float* gS,
                               long npair, long HW, int C, hipStream_t st, bool a16 = false, const float* dE = nullptr, int Ds = 1) {
  long threads = npair * (C / 4);
  dim3 grid((unsigned)((threads + 255) / 256));
  if (dE && (a16 || Ds < 1)) return bad_arg(h, "pixelnorm bwd: dE needs fp32 storage");
#define RD_PNP16(LP) hipLaunchKernelGGL((k_pn_lrelu_bwd_pairs<LP, rd_bf16_t>), grid, dim3(256), 0, st, (const rd_bf16_t*)g, \
                                        (const rd_bf16_t*)hh, rinv, (rd_bf16_t*)dy, (rd_bf16_t*)gS, npair, HW, (const rd_bf16_t*)nullptr, 1)
  if (a16) {
    if (C == 256) RD_PNP16(64); else if (C == 128) RD_PNP16(32); else if (C == 64) RD_PNP16(16);
    else return bad_arg(h, "pixelnorm bwd: C must be 64/128/256");
  }
  else if (C == 256) hipLaunchKernelGGL(k_pn_lrelu_bwd_pairs<64>, grid, dim3(256), 0, st, g, hh, rinv, dy, gS, npair, HW, dE, Ds);
  else if (C == 128) hipLaunchKernelGGL(k_pn_lrelu_bwd_pairs<32>, grid, dim3(256), 0, st, g, hh, rinv, dy, gS, npair, HW, dE, Ds);
  else if (C == 64) hipLaunchKernelGGL(k_pn_lrelu_bwd_pairs<16>, grid, dim3(256), 0, st, g, hh, rinv, dy, gS, npair, HW, dE, Ds);
  else return bad_arg(h, "pixelnorm bwd: C must be 64/128/256");
#undef RD_PNP16
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------
// create / destroy
// ------------------------------------------------------------------------------------

extern "C" int rdgan_create(rdgan_handle** out, int ndomain, int n_cond_channels, int max_batch) {
  if (!out) return -2;
  *out = nullptr;
  if (!rd_geometry_ok(ndomain, n_cond_channels, max_batch)) return -2;
  rdgan_handle* h = new rdgan_handle();      // (zeroed, then the initialisers: from here every failure leaves through rdgan_destroy)
  rd_geometry(h, ndomain, n_cond_channels, max_batch);
  const int nd = ndomain;
  const int* gch = h->gch; const int* dch = h->dch;
  hipError_t e = hipSuccess;
  {
    std::vector<RdRow> tab;
    std::vector<size_t> first;
    if (!rd_build_plans(h, h->plans, tab, first)) { rdgan_destroy(h); return -2; }
    e = hipMalloc((void**)&h->d_tab, sizeof(RdRow) * tab.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_tab, tab.data(), sizeof(RdRow) * tab.size(), hipMemcpyHostToDevice);
    for (int i = 0; i < PL_COUNT; ++i) h->plans[i].tab = h->d_tab + first[i];
  }
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_plans, sizeof(RdPlan) * PL_COUNT);
  if (e == hipSuccess) e = hipMemcpy(h->d_plans, h->plans.data(), sizeof(RdPlan) * PL_COUNT, hipMemcpyHostToDevice);
  if (e != hipSuccess) { rdgan_destroy(h); return (int)e; }

  // workspace carve (two passes: size, then assign)
  const long MB = h->MB, NB = h->NB;
  // partial slabs of the streaming weight-gradient kernels: the worst case over every batch size up to max_batch
  size_t wneed = rd_wgrad_workspace_floats(h, h->plans);
  wneed = std::max(wneed, g9w_partial_floats((int)MB * (RDGAN_NHOURS / 2)));      // k_g9_wgrad_pairs: [27][64] per (sample, plane pair)
  if (g9w_mfma_ok(nd, (long)MB * h->gpix[3]))                              // k_g9_wgrad_mfma: [27][64] per persistent workgroup
    wneed = std::max(wneed, g9w_partial_floats(g9w_groups(true, (int)MB, nd)));
  if (nd == 16) wneed = std::max(wneed, d3w_partial_floats(RD_D3W_GMAX));          // k_d3_wgrad_slab16: [16 groups][27][128][256]
  if (nd % 16 == 0) wneed = std::max(wneed, d2w_partial_floats(RD_D2W_GMAX));      // k_d2_wgrad_slab16 / _t16: [64 groups][27][64][128]
  if (nd == 16) wneed = std::max(wneed, upwgrad2_partial_floats());                // k_upconv2_wgrad_slab16: [8 groups][64][256][128]
  if (nd == 16) wneed = std::max(wneed, upwgrad_partial_floats(RD_UWG_GMAX));      // k_upconv_wgrad_slab16: [32 groups][64][128][64]
  h->wpartial_cap = wneed;
  h->cpartial_cap = (size_t)1024 * std::max(h->n_nodes, 256);
  {  // split-K partials: up to 8 copies of the largest small-M destination (critic layers 3/4, Dense, generator block 1)
    size_t m = std::max<size_t>((size_t)NB * h->dL[3] * 256, (size_t)MB * h->n_nodes);
    m = std::max<size_t>(m, (size_t)NB * h->dL[2] * 128);
    m = std::max<size_t>(m, (size_t)MB * h->gpix[1] * 256);
    h->kpartial_cap = 8 * m;
  }
  for (int pass = 0; pass < 2; ++pass) {
    size_t off = 0;
    auto carve = [&](float*& p, size_t nfloats) {
      off = (off + 255) & ~(size_t)255;
      if (pass == 1) p = (float*)(h->ws + off);
      off += nfloats * sizeof(float);
    };
    carve(h->xcat, MB * h->n_in);
    carve(h->h0, MB * h->gpix[0] * 256);
    carve(h->h1, MB * h->gpix[1] * 256); carve(h->r1, MB * h->gpix[1]);
    carve(h->h2, MB * h->gpix[2] * 128); carve(h->r2, MB * h->gpix[2]);
    carve(h->h3, MB * h->gpix[3] * 64); carve(h->r3, MB * h->gpix[3]);
    carve(h->P9, MB * h->gpix[3] * 32);
    carve(h->fake, MB * h->gpix[3]);
    carve(h->dl, MB * h->gpix[3]);
    carve(h->gh3, MB * h->gpix[3] * 64);
    carve(h->gup3, MB * h->gpix[3] * 128);
    carve(h->dy2, MB * h->gpix[2] * 128);
    carve(h->gup2, MB * h->gpix[2] * 256);
    carve(h->dy1, MB * h->gpix[1] * 256);
    carve(h->gup1, MB * h->gpix[1] * 256);
    carve(h->ga0, MB * h->gpix[0] * 256);
    carve(h->cin, NB * h->dL[0] * h->CP);
    h->dh[0] = nullptr; h->du[0] = nullptr;
    for (int l = 1; l <= 4; ++l) { carve(h->dh[l], NB * h->dL[l] * dch[l]); carve(h->du[l], NB * h->dL[l] * dch[l]); }
    carve(h->v, NB);
    carve(h->P1, MB * h->dL[1] * h->ldp1);
    carve(h->g0, MB * h->dL[0]);
    carve(h->gpv, MB);
    carve(h->wpartial, h->wpartial_cap);
    carve(h->cpartial, h->cpartial_cap);
    carve(h->kpartial, h->kpartial_cap);
    carve(h->kpartial_ahead, h->kpartial_cap);       // (same capacity: the split-K choice tests against kpartial_cap)
    h->DWT[0] = h->DWT[1] = nullptr;
    for (int l = 2; l <= 4; ++l) carve(h->DWT[l], 27L * dch[l - 1] * dch[l]);
    carve(h->W1T, 64 * h->ldp1);
    carve(h->W1P, 27L * h->CP * 64); carve(h->dW1P, 27L * h->CP * 64);
    h->GWT[0] = nullptr;
    for (int l = 1; l <= 3; ++l) carve(h->GWT[l], 27L * gch[l - 1] * gch[l]);
    carve(h->W9T, 64 * 32);
    h->GWC[0] = h->GWD[0] = nullptr;
    for (int l = 1; l <= 3; ++l) { carve(h->GWC[l], 64L * gch[l - 1] * gch[l]); carve(h->GWD[l], 64L * gch[l - 1] * gch[l]); }
    carve(h->dWc, 64L * 256 * 256);
    {
      size_t ne = 0, ns = 0;
      for (int l = 1; l <= 3; ++l) {
        const int* sd = h->gdim[l - 1];
        ne = std::max(ne, (size_t)(sd[0] + 1) * sd[1] * sd[2] * gch[l - 1]);
        ns = std::max(ns, (size_t)sd[0] * 4 * sd[1] * sd[2] * gch[l]);
      }
      h->fE[0] = h->fU[0] = nullptr;
      for (int l = 1; l <= 3; ++l) {
        const int* sd = h->gdim[l - 1];
        carve(h->fE[l], MB * (size_t)(sd[0] + 1) * sd[1] * sd[2] * gch[l - 1]);
        carve(h->fU[l], 48L * gch[l - 1] * gch[l]);
      }
      carve(h->fdE, MB * ne); carve(h->fgS, MB * ns);
      {   // bf16 weight images (2 bytes per element: half the floats)
        float* p = nullptr;
        h->bU[0] = nullptr;
        for (int l = 1; l <= 3; ++l) { carve(p, 24L * gch[l - 1] * gch[l] + 8); h->bU[l] = p; }
        carve(p, 24L * 256 * 256 + 8); h->bUT = p;
        const long KP128 = (h->n_in + 127) / 128 * 128;                               // (the skinny Dense kernel's images: K in whole 128s)
        carve(p, (long)((MB + 31) / 32 * 32) * KP128 / 2 + 8); h->xcat16 = p;         // (whole 32-row blocks)
        carve(p, (long)h->n_nodes * KP128 / 2 + 8); h->bW0 = p;
        h->bWF[0] = h->bWF[1] = h->bWB[0] = h->bWB[1] = nullptr;
        for (int l = 2; l <= 4; ++l) {
          carve(p, 27L * dch[l - 1] * dch[l] / 2 + 8); h->bWF[l] = p;
          carve(p, 27L * dch[l - 1] * dch[l] / 2 + 8); h->bWB[l] = p;
        }
        h->bG1F[0] = nullptr;
        for (int l = 1; l <= 3; ++l) { carve(p, 32L * gch[l - 1] * gch[l] + 8); h->bG1F[l] = p; }
        carve(p, 32L * 256 * 256 + 8); h->bG1B = p;
        h->fWF[0] = h->fWF[1] = h->fWB[0] = h->fWB[1] = h->fG1F[0] = nullptr;
        for (int l = 2; l <= 4; ++l) {
          carve(p, 27L * dch[l - 1] * dch[l] / 2 + 8); h->fWF[l] = p;
          carve(p, 27L * dch[l - 1] * dch[l] / 2 + 8); h->fWB[l] = p;
        }
        for (int l = 1; l <= 3; ++l) { carve(p, 32L * gch[l - 1] * gch[l] + 8); h->fG1F[l] = p; }
        carve(p, 32L * 256 * 256 + 8); h->fG1B = p;
        carve(p, 32L * h->ldp1 + 8); h->bW1B = p;
        carve(p, 64L * 8 * 2 * 64 * 4 + 8); h->bW3I = p;
        carve(p, 64L * 8 * 2 * 64 * 4 + 8); h->bW3T = p;
        carve(p, 4L * 64 * 4 + 8); h->bW9I = p;
        carve(p, (long)RD_UP2_KSTEPS * 4 * 64 * 4 + 8); h->bW2I = p;
        carve(p, (long)RD_D2S_KSTEPS * 2 * 64 * 4 + 8); h->bW2S = p;
        if (nd % 16 == 0) { carve(p, NB * h->dL[1] * 4 + 8); if (pass == 1) h->g1bits = (unsigned char*)p; }     // (the domains with a layer-2 input-gradient slab kernel)
        carve(p, (long)RD_D2F_KSTEPS * 4 * 64 * 4 + 8); h->bW2F = p;
      }
      carve(h->fdU, 48L * 256 * 256); carve(h->fUT, 48L * 256 * 256);
    }
    { float* f = nullptr; carve(f, 64); if (pass == 1) { h->d_flag = (int*)f; h->flag_ahead = (int*)f + 32; } }
    carve(h->g9b_tmp, 64);
    carve(h->ubias_part, 32 * 8 * 64);
    carve(h->gp_part, (size_t)MB * 64);
    carve(h->dw6_part, (size_t)16 * h->F);
    if (pass == 0) {
      h->ws_bytes = off + 256;
      e = hipMalloc((void**)&h->ws, h->ws_bytes);
      if (e != hipSuccess) { rdgan_destroy(h); return (int)e; }
      (void)hipMemset(h->ws, 0, h->ws_bytes);
    }
  }
  // side stream + ordering events (no timing); failure to create them only turns the option off
  {
    bool ok = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) == hipSuccess;
    hipEvent_t* evs[] = {&h->ev_fork, &h->ev_join, &h->ev_cw, &h->ev_g[1], &h->ev_g[2], &h->ev_g[3]};
    for (hipEvent_t* e2 : evs) ok = ok && hipEventCreateWithFlags(e2, hipEventDisableTiming) == hipSuccess;
    if (!ok) { h->side_on = 0; (void)hipGetLastError(); }
    // the early generator forward's stream: a compute stream of its own (not the side stream, whose weight forms and column
    // sums must not queue behind a 2 ms forward)
    bool ok2 = hipStreamCreateWithFlags(&h->ahead, hipStreamNonBlocking) == hipSuccess;
    ok2 = ok2 && hipEventCreateWithFlags(&h->ev_ahead_fork, hipEventDisableTiming) == hipSuccess;
    ok2 = ok2 && hipEventCreateWithFlags(&h->ev_ahead_done, hipEventDisableTiming) == hipSuccess;
    if (!ok2) { h->ahead = nullptr; (void)hipGetLastError(); }
  }
  *out = h;
  return 0;
}

extern "C" void rdgan_destroy(rdgan_handle* h) {
  if (!h) return;
  if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
  if (h->ahead) { (void)hipStreamSynchronize(h->ahead); (void)hipStreamDestroy(h->ahead); }
  for (hipEvent_t e2 : {h->ev_fork, h->ev_join, h->ev_cw, h->ev_g[1], h->ev_g[2], h->ev_g[3], h->ev_ahead_fork, h->ev_ahead_done})
    if (e2) (void)hipEventDestroy(e2);
  for (auto& r : h->launch_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (int t = 0; t < RDGAN_NUM_TAGS; ++t) {
    for (auto e : h->ev_start[t]) (void)hipEventDestroy(e);
    for (auto e : h->ev_stop[t]) (void)hipEventDestroy(e);
  }
  for (void* g : h->gate_keep) if (g) (void)hipFree(g);
  if (h->ws) (void)hipFree(h->ws);
  if (h->d_plans) (void)hipFree(h->d_plans);
  if (h->d_tab) (void)hipFree(h->d_tab);
  delete h;
}

extern "C" const char* rdgan_last_error(const rdgan_handle* h) { return h ? h->err.c_str() : "null handle"; }
extern "C" long rdgan_gen_param_count(const rdgan_handle* h) { return h ? h->n_gen : -1; }
extern "C" long rdgan_critic_param_count(const rdgan_handle* h) { return h ? h->n_critic : -1; }
extern "C" long rdgan_workspace_bytes(const rdgan_handle* h) { return h ? (long)h->ws_bytes : -1; }
extern "C" int rdgan_gen_param_layout(const rdgan_handle* h, long* offsets, long* sizes) {
  if (!h) return -2;
  for (int i = 0; i < 10; ++i) { if (offsets) offsets[i] = h->goff[i]; if (sizes) sizes[i] = h->gsz[i]; }
  return 10;
}
extern "C" int rdgan_critic_param_layout(const rdgan_handle* h, long* offsets, long* sizes) {
  if (!h) return -2;
  for (int i = 0; i < 10; ++i) { if (offsets) offsets[i] = h->doff[i]; if (sizes) sizes[i] = h->dsz[i]; }
  return 10;
}

// bf16 storage mode: its last conv exists only as the direct kernel, which keeps 4 (ndomain + 2)^2 floats in LDS -- ndomain <= 72
static bool a16_geometry_ok(int nd) { return 4 * (size_t)(nd + 2) * (nd + 2) * sizeof(float) <= 96 * 1024; }
#define RD_A16_TOO_LARGE "bf16 storage mode: ndomain too large (the mode supports ndomain <= 72; fp32 storage runs every accepted ndomain)"

// ---- what setting an option does beyond its table row (RD_OPTIONS, rdgan_options.h)
// "bf16": refused here, not at the first step, on a geometry the mode does not support: the mode stays off
static int opt_bf16_admit(rdgan_handle* h, int v) {
  return v && !a16_geometry_ok(h->nd) ? bad_arg(h, RD_A16_TOO_LARGE) : 0;
}
// "side_stream": on only where the stream exists
static int opt_side_stream_value(const rdgan_handle* h, int v) { return (v && h->side) ? 1 : 0; }
// "keep_gates": the copies are allocated when the option is set, never inside a step
static int opt_keep_gates_buffers(rdgan_handle* h) {
  h->gate_keep_B = 0;
  for (int l = 1; l <= 4 && h->keep_gates; ++l)
    if (!h->gate_keep[l]) RD_CHECK(h, hipMalloc(&h->gate_keep[l], (size_t)h->MB * h->dL[l] * h->dch[l] * sizeof(float)));
  return 0;
}

// (an option that shapes weight forms needs nothing here: its row's flag puts it into rd_form_key, which the form builders compare)
extern "C" int rdgan_set_option(rdgan_handle* h, const char* name, int value) {
  if (!h || !name) return -2;
  const RdOptionRow* row = rd_option_find(name);
  if (!row) return bad_arg(h, "set_option: unknown option");
  int v = 0;
  if (!rd_option_normalise(*row, value, &v)) return bad_arg(h, row->refusal);      // ("conv_f16", "sample_offset": their messages)
  if (row->field == &RdOptions::a16) RD_TRY(opt_bf16_admit(h, v));
  if (row->field == &RdOptions::side_on) v = opt_side_stream_value(h, v);
  h->*(row->field) = v;
  if (row->field == &RdOptions::keep_gates) return opt_keep_gates_buffers(h);
  return 0;
}

extern "C" int rdgan_set_weight_versions(rdgan_handle* h, uint64_t gen_version, uint64_t critic_version) {
  if (!h) return -2;
  h->gver_in = gen_version; h->cver_in = critic_version;
  return 0;
}
extern "C" int rdgan_form_builds(const rdgan_handle* h, long* gen_builds, long* critic_builds) {
  if (!h) return -2;
  if (gen_builds) *gen_builds = h->form_builds[0];
  if (critic_builds) *critic_builds = h->form_builds[1];
  return 0;
}

extern "C" int rdgan_profile(rdgan_handle* h, unsigned tag_mask) {
  if (!h) return -2;
  h->prof_mask = tag_mask;
  for (int t = 0; t < RDGAN_NUM_TAGS; ++t) {
    h->ev_used[t] = 0;
    if ((tag_mask >> t & 1u) && h->ev_start[t].empty()) {
      h->ev_start[t].resize(4096); h->ev_stop[t].resize(4096);
      for (size_t i = 0; i < 4096; ++i) {
        RD_CHECK(h, hipEventCreate(&h->ev_start[t][i]));
        RD_CHECK(h, hipEventCreate(&h->ev_stop[t][i]));
      }
    }
  }
  return 0;
}
static const char* const RD_PLAN_NAMES[PL_COUNT] = {
  "gen dense", "gen block1 fwd (direct)", "gen block2 fwd (direct)", "gen block3 fwd (direct)", "gen conv 64->1 fwd", "gen block1 dgrad (direct)",
  "gen block2 dgrad (direct)", "gen block3 dgrad (direct)", "gen conv 64->1 bwd",
  "critic layer1", "critic layer2", "critic layer3", "critic layer4", "critic layer2 dgrad", "critic layer3 dgrad", "critic layer4 dgrad",
  "critic layer1 dgrad (column GEMM)",
  "gen block1 (collapsed)", "gen block2 (collapsed)", "gen block3 (collapsed)", "gen block1 dgrad (collapsed)", "gen block2 dgrad (collapsed)",
  "gen block3 dgrad (collapsed)",
  "gen block1 shared-centre E[s]", "gen block2 shared-centre E[s]", "gen block3 shared-centre E[s]",
  "gen block1 shared-centre S", "gen block2 shared-centre S", "gen block3 shared-centre S",
  "gen block1 shared-centre E[s+1]", "gen block2 shared-centre E[s+1]", "gen block3 shared-centre E[s+1]",
  "gen block1 dgrad shared part", "gen block2 dgrad shared part", "gen block3 dgrad shared part",
  "gen block1 dgrad difference part", "gen block2 dgrad difference part", "gen block3 dgrad difference part",
  "gen block1 fwd difference part", "gen block2 fwd difference part", "gen block3 fwd difference part",
  "critic layer2 (border boxes)", "critic layer3 (border boxes)", "critic layer4 (border boxes)",
  "critic layer2 dgrad (border boxes)", "critic layer3 dgrad (border boxes)", "critic layer4 dgrad (border boxes)",
  "gen block1 shared-centre E[s] (boxes)", "gen block2 shared-centre E[s] (boxes)", "gen block3 shared-centre E[s] (boxes)",
  "gen block1 shared-centre S (boxes)", "gen block2 shared-centre S (boxes)", "gen block3 shared-centre S (boxes)",
  "gen block1 shared-centre E[s+1] (boxes)", "gen block2 shared-centre E[s+1] (boxes)", "gen block3 shared-centre E[s+1] (boxes)",
  "gen block1 (collapsed, boxes)", "gen block2 (collapsed, boxes)", "gen block3 (collapsed, boxes)",
  "gen block1 dgrad (collapsed, boxes)", "gen block2 dgrad (collapsed, boxes)", "gen block3 dgrad (collapsed, boxes)",
  "gen dense (bf16 pipe)"};

extern "C" int rdgan_profile_launches(rdgan_handle* h, int on) {
  if (!h) return -2;
  if (on && h->launch_recs.empty()) {
    h->launch_recs.resize(8192);
    for (auto& r : h->launch_recs) { RD_CHECK(h, hipEventCreate(&r.e0)); RD_CHECK(h, hipEventCreate(&r.e1)); }
  }
  h->prof_launches = on ? 1 : 0;
  if (on) h->launch_used = 0;
  return 0;
}
extern "C" int rdgan_launch_table(rdgan_handle* h, rdgan_launch_stat* out, int cap, int* n_out) {
  if (!h || !out || cap < 1 || !n_out) return -2;
  RD_CHECK(h, hipDeviceSynchronize());
  int n = 0;
  for (size_t i = 0; i < h->launch_used; ++i) {
    const RdLaunchRec& r = h->launch_recs[i];
    float ms = 0;
    RD_CHECK(h, hipEventElapsedTime(&ms, r.e0, r.e1));
    int k = 0;
    for (; k < n; ++k)
      if (out[k].plan == r.plan && out[k].kind == r.kind && out[k].batch == r.batch && !strcmp(out[k].kernel, r.kernel)) break;
    if (k == n) {
      if (n == cap) continue;
      memset(&out[n], 0, sizeof(out[n]));
      out[n].plan = r.plan; out[n].kind = r.kind; out[n].batch = r.batch;
      memcpy(out[n].kernel, r.kernel, sizeof(r.kernel));
      snprintf(out[n].name, sizeof(out[n].name), "%s", r.plan >= 0 && r.plan < PL_COUNT ? RD_PLAN_NAMES[r.plan] : "op");
      ++n;
    }
    out[k].launches += 1; out[k].gflop += r.flops * 1e-9; out[k].ms += ms;
  }
  *n_out = n;
  return 0;
}

extern "C" int rdgan_flop_count(rdgan_handle* h, double* flops, int reset) {
  if (!h) return -2;
  if (flops) *flops = h->flops_acc;
  if (reset) h->flops_acc = 0;
  return 0;
}
extern "C" int rdgan_profile_read(rdgan_handle* h, int tag, double* total_ms, long* launches) {
  if (!h || tag < 0 || tag >= RDGAN_NUM_TAGS) return -2;
  RD_CHECK(h, hipDeviceSynchronize());
  double tot = 0;
  for (size_t i = 0; i < h->ev_used[tag]; ++i) {
    float ms = 0;
    RD_CHECK(h, hipEventElapsedTime(&ms, h->ev_start[tag][i], h->ev_stop[tag][i]));
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (long)h->ev_used[tag];
  return 0;
}

// ------------------------------------------------------------------------------------
// generator forward (T:312-357)
// ------------------------------------------------------------------------------------
static RdEpi epi_make(int mode, const float* bias = nullptr, const float* aux = nullptr, int use_drop = 0,
                      uint32_t key = 0, uint32_t idx_base = 0) {
  RdEpi e; e.mode = mode; e.use_drop = use_drop; e.key = key; e.idx_base = idx_base; e.bias = bias; e.aux = aux;
  e.ksplit = 1; e.kpart = nullptr; e.kstride = 0; e.rinv = nullptr; e.gw = e.ghw = e.gq = 0;
  e.addt = nullptr; e.addt_plane = 0; e.nametag = 0; e.out16 = 0;
  return e;
}
// pointer arithmetic on an activation tensor of the workspace: bf16 elements in the storage mode, floats otherwise
static inline float* act_off(const rdgan_handle* h, float* p, long elems) {
  return (float*)((char*)p + elems * (h->a16 ? 2 : 4));
}
// bf16 storage mode needs the forms whose GEMMs all exist as bf16 kernels
static int a16_check(rdgan_handle* h) {
  if (!h->a16) return 0;
  if (!h->collapse || !h->g9_direct)
    return bad_arg(h, "bf16 storage mode needs the options collapse and g9_direct at 1");
  if (!a16_geometry_ok(h->nd)) return bad_arg(h, RD_A16_TOO_LARGE);
  return 0;
}

// the shared-centre form pays where the hour axis of the block input is long enough for its (D+1)/D boundary plane
// "fast_fwd" / "fast_bwd" at their default (-1) follow the storage mode: the shared-centre form saves a quarter of the tap
// products, which pays where the matrix pipe is the bound (fp32: 64 FLOP/clk/SIMD); with bf16 operands the pipe is 16x faster
// and nowhere near busy, so the plain collapsed form wins there -- one GEMM per block instead of two, no hour-difference /
// plane-sum / recombination passes (measured at bs 256: 3.89 vs 4.09 ms per iteration)
static int fast_fwd_on(const rdgan_handle* h) { return h->fast_fwd < 0 ? !h->a16 : h->fast_fwd; }
static int fast_bwd_on(const rdgan_handle* h) { return h->fast_bwd < 0 ? !h->a16 : h->fast_bwd; }
static bool gen_block_fast(const rdgan_handle* h, int l, int enabled) {
  return h->collapse && enabled && h->gdim[l - 1][0] >= 6;
}

// generator block 3 forward by the slab kernel (rdgan_upconv16.hip.h): bf16 storage mode, collapsed form, the 12 x 8 x 8 x 128
// -> 24 x 16 x 16 x 64 block of ndomain 16
static bool upconv_slab_on(const rdgan_handle* h, int l) {
  return h->upconv_slab && h->a16 && h->collapse && l == 3 && h->nd == 16 && !gen_block_fast(h, 3, fast_fwd_on(h));
}
// the same block on (h, w) tiles of 8 x 8 source positions with their halo (rdgan_upconv16t.hip.h): source planes of 16 x 16, 32 x 32, ...
static bool upconv_slab_t_on(const rdgan_handle* h, int l) {
  return h->upconv_slab_t && h->a16 && h->collapse && l == 3 && h->nd > 16 && h->gdim[2][1] % 8 == 0 && h->gdim[2][2] % 8 == 0 &&
         h->bW3T && !gen_block_fast(h, 3, fast_fwd_on(h));
}
static bool upconv2_slab_on(const rdgan_handle* h, int l) {
  return h->upconv2_slab && h->a16 && h->collapse && l == 2 && h->nd == 16 && !gen_block_fast(h, 2, fast_fwd_on(h));
}

// plan of the forward / second-sweep GEMM of critic layer l >= 2 over n samples: the border-class boxes where they pay -- with
// few rows the boxes' short tap lists lose the K splits that fill the chip (layer 3 at 256 samples: 60 -> 68 us), so a small
// launch keeps the one-phase plan unless the boxes drop more than half of the work (layer 4: 70 %)
static int critic_box_plan(const rdgan_handle* h, int one, int box, long rows) {
  if (!h->border_boxes || !h->plans[box].boxes) return one;
  if (std::max(h->plans[box].src_sample, h->plans[box].dst_sample) * 4 * 258 >= 0x7FFFFFF0L) return one;      // (32-bit offsets of a tile)
  if (h->border_boxes >= 2 || rows >= 8192 || 2.0 * plan_flops(h->plans[box], 1) <= plan_flops(h->plans[one], 1)) return box;
  return one;
}
static int critic_fwd_plan(const rdgan_handle* h, int l, int n) {
  return critic_box_plan(h, PL_D2F + l - 2, PL_D2FX + l - 2, (long)n * h->dL[l]);
}
// weight gradient of layer l >= 2 (streaming kernels): every box is its own set of partial slabs and short-K workgroups, so the
// boxes must drop at least 30 % of the work to pay (ndomain 64, layer 3: 18 % dropped, 0.130 -> 0.142 ms)
static int critic_wgrad_plan(const rdgan_handle* h, int l, int n) {
  const int one = PL_D2F + l - 2, box = PL_D2FX + l - 2;
  if (!h->wgrad_boxes || !wgrad_box_ok(h->plans[box])) return one;
  if (h->border_boxes < 2 && plan_flops(h->plans[box], 1) > 0.7 * plan_flops(h->plans[one], 1)) return one;
  return critic_fwd_plan(h, l, n);
}
// the same choice for the input gradient of layer l >= 2 (rows = the layer's input positions)
static int critic_dgrad_plan(const rdgan_handle* h, int l, int n) {
  return critic_box_plan(h, PL_D2B + l - 2, PL_D2BX + l - 2, (long)n * h->dL[l - 1]);
}

// collapsed generator block (forward or input gradient): the border-class boxes where the launch runs several rounds of workgroups
// -- in a single round the interior box's workgroups, which keep every tap, set the time -- and the boxes drop 30 % of the work
// (block 1, 3 x 2 x 2 source grid: 47 % of its row-tap products are products with a zero row; blocks 2 / 3: 30 % / 16 %)
static bool box_span_ok(const RdPlan& p, int B) {      // a tile of the smallest box must stay inside the kernels' 32-bit offsets
  long minL = p.ph[0].L;
  for (int i = 1; i < p.nphases; ++i) minL = std::min<long>(minL, p.ph[i].L);
  return std::min<long>(B, 256 / minL + 2) * std::max(p.src_sample, p.dst_sample) * 4 < 0x7FFFFFF0L;
}
static int gen_box_plan(const rdgan_handle* h, int one, int box, int B) {
  if (!h->border_boxes || !h->plans[box].boxes || !box_span_ok(h->plans[box], B)) return one;
  if (h->border_boxes >= 2) return box;
  if (plan_flops(h->plans[box], 1) > 0.7 * plan_flops(h->plans[one], 1)) return one;
  return plan_tiles(h->plans[one], B, 128) * (h->plans[one].N / 128 > 0 ? h->plans[one].N / 128 : 1) >= 1024 ? box : one;
}

// the Dense layer by k_dense16_skinny (rdgan_edge.hip.h): the weight image is then in fragment order, so the choice is made per
// HANDLE (every call has B <= max_batch <= 128), not per call
static int dense_skinny_ks(const rdgan_handle* h) { return (h->n_in + 127) / 128 * 8; }      // k-steps of 16, a multiple of 8 (two waves x sets of four)
static bool dense_skinny_on(const rdgan_handle* h) {
  return h->a16 && h->dense16 && h->dense_skinny && h->MB <= 128 && h->bW0 && h->xcat16 && h->n_nodes % 32 == 0 && h->KP0 % 64 == 0;
}
static bool g9_fused_on(const rdgan_handle* h) { return h->g9_fused && h->tapgather && upconv_slab_on(h, 3); }
// the same inside the TILED block-3 kernel (ndomain 32, 64: k_upconv_slab_t16<G9>, k_tapsum_softmax12t)
static bool g9_fused_t_on(const rdgan_handle* h) { return h->g9_fused && h->tapgather && upconv_slab_t_on(h, 3); }
// the Dense layer on the bf16 matrix pipe, a third of the columns per launch (the skinny kernel goes first where it is on): at
// ndomain 64 its 825 MB fp32 kernel is the launch (HBM-bound); the bf16 image halves it
static bool dense16_on(const rdgan_handle* h) { return h->a16 && h->dense16 && h->dense16_ok && h->bW0 && h->xcat16; }

// ---- routes of the generator step's backward
// weight gradient of a generator block (collapsed form, or one tap group of the shared-centre form) through the streaming kernels
// on the (h, w) border boxes `box` of plan `one` (12 % of a block's row-tap products are products with a zero row) -- where they
// drop at least a fifth of the work (block 2: 23 %, 0.237 -> 0.219 ms per launch; block 3's 12 % do not pay for the extra partial
// slabs and short row tiles of its 256 x 64 tiling: 0.43 -> 0.51 ms, measured)
static bool gen_wgrad_boxes_on(const rdgan_handle* h, int one, int box) {
  return h->wgrad_boxes && h->border_boxes && h->wave_spec && wgrad_box_ok(h->plans[box]) &&
         (h->border_boxes >= 2 || plan_flops(h->plans[box], 1) < 0.8 * plan_flops(h->plans[one], 1));
}
// weight gradient (and bias gradient) of collapsed block 3 / block 2 by k_upconv_wgrad_slab16 / k_upconv2_wgrad_slab16: bf16
// storage mode, ndomain 16
static bool upwgrad_slab_on(const rdgan_handle* h, int l) { return h->a16 && (l == 3 || l == 2) && h->upwgrad_slab && h->nd == 16; }
// Backward of the 64 -> 1 conv in its direct form: straight from the 1-channel dlogits with the four neighbouring hour planes in
// LDS -- no im2col matrix, and the input gradient goes through block 3's PixelNorm+LeakyReLU backward in the same kernel; needs
// the planes to fit in LDS and the weight gradient's partial rows in the workspace
static size_t g9_pairs_lds(const rdgan_handle* h) { return 4 * (size_t)(h->nd + 2) * (h->nd + 2) * sizeof(float); }
static bool g9_direct_on(const rdgan_handle* h, int B) {
  return h->g9_direct && g9_pairs_lds(h) <= 96 * 1024 && g9w_partial_floats(B * (RDGAN_NHOURS / 2)) <= h->wpartial_cap;
}
// ... with exact fp32 products on the matrix pipe and the row's backward in registers (k_g9_bwd_mfma16, rdgan_g9bwd16.hip.h): bf16
// storage mode, block 3 in the collapsed form (the shared-centre form also wants the plane-pair sums, which k_g9_bwd_pairs leaves)
static bool g9_bwd_mfma_on(const rdgan_handle* h) {
  return h->a16 && !gen_block_fast(h, 3, fast_bwd_on(h)) && h->g9_bwd_mfma && (h->nd * h->nd) % 32 == 0;
}

// What the stages of one pass over the generator share, built once per call: bf16 storage mode, collapsed form, the last conv's
// backward in its direct form (g9_direct_on); per block l its output hs[l] and PixelNorm's 1/l2 rs[l]; backward: the gradient wrt
// its conv output dys[l] and wrt its input gups[l] (direct form: on the upsampled grid; collapsed: on the source grid)
struct GenPass { bool a16; int col; bool g9_direct; float *hs[4], *rs[4], *dys[4], *gups[4]; };
static GenPass gen_pass(const rdgan_handle* h, int B) {
  return {h->a16 != 0, h->collapse, g9_direct_on(h, B), {h->h0, h->h1, h->h2, h->h3}, {nullptr, h->r1, h->r2, h->r3},
          {nullptr, h->dy1, h->dy2, h->gh3}, {nullptr, h->gup1, h->gup2, h->gup3}};
}

// hour differences E of a block input (shared-centre form): forward, and the backward of a block whose forward ran another form
static void launch_diff_d(const GenPass& s, const float* x, float* E, int B, int D, long P, hipStream_t st) {
  launch_diff_d(s.a16, x, E, B, D, P, st);
}
// epilogue of the last conv where the GEMM / streaming kernel has left gq = 3 (9) in-tile tap sums per grid point in P9: the
// remaining sums, bias, Softmax(axis=1), check_numerics
static void launch_tapsum_softmax(rdgan_handle* h, int gq, float* out, const float* gp, int B, hipStream_t st) {
  launch_tapsum_softmax_q(gq, h->P9, gp + h->goff[9], out, B, h->nd, h->nd, h->d_flag, st);
}

// Weight forms (read only the weights), on `ws`: skipped when the caller vouches that the forms in the workspace were built from
// these very weights (same slab, same content version, same form options).  *built: the form kernels were issued.
static int gen_build_forms(rdgan_handle* h, const float* gp, hipStream_t st, hipStream_t ws, bool* built) {
  const bool a16 = h->a16 != 0;
  const int gcfg = rd_form_key(h, RD_FORMS_GEN);       // every option this function reads, directly or through a predicate
  *built = !(h->gver_in != 0 && gp == h->gcache_ptr && h->gver_in == h->gcache_ver && gcfg == h->gcache_cfg);
  if (!*built) return 0;
  h->form_builds[0]++;
  h->gcache_ptr = nullptr; h->gcache_ver = 0; h->gcache_cfg = -1;     // (valid again only once every form kernel has been issued)
  // W9T [64][32] = W9[tap][ci]^T (zero padded taps 27..31)
  RD_TRY(launch_transpose(h, gp + h->goff[8], h->W9T, 1, 27, 64, 32, ws));
  if (dense_skinny_on(h)) {
    const long nimg = (long)(h->n_nodes / 32) * dense_skinny_ks(h) * 16;      // (threads: four lanes' fragments each)
    hipLaunchKernelGGL(k_dense_wimg, dim3((unsigned)((nimg + 255) / 256)), dim3(256), 0, ws, gp + h->goff[0], (unsigned short*)h->bW0,
                       h->n_in, h->n_nodes, dense_skinny_ks(h));
  } else if (dense16_on(h)) hipLaunchKernelGGL(k_dense_w16, dim3((h->n_nodes + 31) / 32, (h->KP0 + 31) / 32), dim3(256), 0, ws, gp + h->goff[0],
                       (unsigned short*)h->bW0, h->n_in, h->n_nodes, h->KP0);
  if (g9_fused_on(h) || g9_fused_t_on(h)) hipLaunchKernelGGL(k_g9_wimg, dim3(1), dim3(256), 0, ws, gp + h->goff[8], (unsigned short*)h->bW9I);
  for (int l = 1; l <= 3; ++l) {
    const float* Wl = gp + h->goff[2 * l];
    const long cc = (long)h->gch[l - 1] * h->gch[l];
    if (gen_block_fast(h, l, fast_fwd_on(h))) {
      ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, ws);
      launch_weight_transform(Wl, h->fU[l], cc, ws);
      if (a16) RD_TRY(launch_weights_to_bf16_t(h, h->fU[l], h->bU[l], 48, h->gch[l - 1], h->gch[l], ws));
    } else if (h->collapse) {
      launch_collapse_weights(Wl, h->GWC[l], cc, ws);
      if (upconv_slab_on(h, l)) launch_upconv_wimg(h->GWC[l], h->bW3I, ws);
      else if (upconv_slab_t_on(h, l)) launch_upconv_wimg_t(h->GWC[l], h->bW3T, ws);
      else if (upconv2_slab_on(h, l)) launch_upconv2_wimg(h->GWC[l], h->bW2I, ws);
      else if (a16) RD_TRY(launch_weights_to_bf16_t(h, h->GWC[l], h->bG1F[l], 64, h->gch[l - 1], h->gch[l], ws, h->conv_f16 ? h->fG1F[l] : nullptr));
    }
    if (ws != st) RD_CHECK(h, hipEventRecord(h->ev_g[l], ws));
  }
  RD_CHECK(h, hipGetLastError());
  h->gcache_ptr = gp; h->gcache_ver = h->gver_in; h->gcache_cfg = gcfg;
  return 0;
}

// concat, then Dense + LeakyReLU (T:326-327); the Reshape (T:328) is a view.  wait_forms: the weight forms were built on another
// stream by this call (the Dense images are built in front of block 1's forms: behind ev_g[1])
static int gen_dense_fwd(rdgan_handle* h, const GenPass& s, const float* gp, const float* z, const float* cond, int B, bool wait_forms, hipStream_t st) {
  const int nd = h->nd;
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    const bool d16 = dense16_on(h) && !dense_skinny_on(h);
    hipLaunchKernelGGL(k_concat, dim3(ew_blocks((long)B * h->n_in)), dim3(256), 0, st, z, cond, h->xcat, B,
                       RDGAN_LATENT_DIM, nd * nd * h->nc, h->d_flag,       // (first kernel of every entry: clears the non-finite flag)
                       d16 ? (unsigned short*)h->xcat16 : (unsigned short*)nullptr, h->KP0);
  }
  if (dense_skinny_on(h)) {
    // small batch: the kernel is the launch (415 MB of bf16 weights at ndomain 64) -- weights and input rows streamed in fragment order
    if (wait_forms) RD_CHECK(h, hipStreamWaitEvent(st, h->ev_g[1], 0));
    const int RB = (B + 31) / 32, KS = dense_skinny_ks(h);
    ProfScope ps(h, -1, st);
    LaunchScope ls(h, PL_GDENSE16, RD_KIND_CONV, B, 3.0 * plan_flops(h->plans[PL_GDENSE16], B), st);
    RD_KNAME(h, "k_dense16_skinny<bf16>");
    h->flops_acc += 3.0 * plan_flops(h->plans[PL_GDENSE16], B);         // (the plan is a third of the columns)
    hipLaunchKernelGGL(k_concat16f, dim3((unsigned)(((long)KS * RB * 64 + 255) / 256)), dim3(256), 0, st, z, cond, (unsigned short*)h->xcat16, B,
                       RDGAN_LATENT_DIM, nd * nd * h->nc, KS, RB);
    const dim3 dg((unsigned)(h->n_nodes / 32));
    const unsigned short* xi = (const unsigned short*)h->xcat16; const unsigned short* wi = (const unsigned short*)h->bW0;
    const float* bs = gp + h->goff[1];
    if (RB == 1) hipLaunchKernelGGL(k_dense16_skinny<1>, dg, dim3(128), 0, st, xi, wi, bs, (rd_bf16_t*)h->h0, B, KS, h->n_nodes);
    else if (RB == 2) hipLaunchKernelGGL(k_dense16_skinny<2>, dg, dim3(128), 0, st, xi, wi, bs, (rd_bf16_t*)h->h0, B, KS, h->n_nodes);
    else if (RB == 3) hipLaunchKernelGGL(k_dense16_skinny<3>, dg, dim3(128), 0, st, xi, wi, bs, (rd_bf16_t*)h->h0, B, KS, h->n_nodes);
    else hipLaunchKernelGGL(k_dense16_skinny<4>, dg, dim3(128), 0, st, xi, wi, bs, (rd_bf16_t*)h->h0, B, KS, h->n_nodes);
    RD_CHECK(h, hipGetLastError());
  } else if (dense16_on(h)) {
    if (wait_forms) RD_CHECK(h, hipStreamWaitEvent(st, h->ev_g[1], 0));
    const int n3 = h->n_nodes / 3;
    for (int j = 0; j < 3; ++j) {
      RdEpi ed = epi_make(RD_EPI_BIAS_LRELU, gp + h->goff[1] + (long)j * n3);
      ed.out16 = 1;
      const unsigned short* wj = (const unsigned short*)h->bW0 + (long)j * n3 * h->KP0;
      float* dj = (float*)((rd_bf16_t*)h->h0 + (long)j * n3);
      if (B <= 128) {       // one row tile: the 64-column tile doubles the workgroups that stream the kernel (ndomain 64: 138 MB per launch)
        ProfScope ps(h, -1, st);
        LaunchScope ls(h, PL_GDENSE16, RD_KIND_CONV, B, plan_flops(h->plans[PL_GDENSE16], B), st);
        h->flops_acc += plan_flops(h->plans[PL_GDENSE16], B);
        RD_TRY((launch_conv_ws_cfg<128, 64, 2, 2, true>(h, h->plans[PL_GDENSE16], h->d_plans + PL_GDENSE16, B, (const float*)h->xcat16,
                                                        (const float*)wj, 0, dj, ed, st)));
      } else RD_TRY(launch_conv16(h, h->plans[PL_GDENSE16], h->d_plans + PL_GDENSE16, B, h->xcat16, wj, dj, ed, st, -1));
    }
  } else if (s.a16) RD_TRY(launch_conv_a16(h, h->plans[PL_GDENSE], h->d_plans + PL_GDENSE, B, h->xcat, gp + h->goff[0], h->n_nodes, h->h0,
                           epi_make(RD_EPI_BIAS_LRELU, gp + h->goff[1]), st, -1, false, true));
  else RD_TRY(launch_conv(h, h->plans[PL_GDENSE], h->d_plans + PL_GDENSE, B, h->xcat, gp + h->goff[0], h->n_nodes, h->h0,
                       epi_make(RD_EPI_BIAS_LRELU, gp + h->goff[1]), st, -1));
  return 0;
}

// block l in the shared-centre form along the hour axis: T = S x[s] once per output plane pair, then the difference part
static int gen_block_fwd_shared_centre(rdgan_handle* h, const GenPass& s, const float* gp, int l, int B, hipStream_t st) {
  const bool a16 = s.a16;
  const int* sd = h->gdim[l - 1];
  const int tag = l == 3 ? RDGAN_TAG_GCONV3_FWD : RDGAN_TAG_GCONV_FWD;
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_diff_d(s, s.hs[l - 1], h->fE[l], B, sd[0], (long)sd[1] * sd[2] * h->gch[l - 1], st);
  }
  const int pls = PL_F1WS + l - 1, ple = PL_F1FE + l - 1;
  RdEpi et = epi_make(RD_EPI_PLAIN);
  et.out16 = a16;
  if (a16) RD_TRY(launch_conv16(h, h->plans[pls], h->d_plans + pls, B, s.hs[l - 1], h->bU[l], h->fgS, et, st, RDGAN_TAG_GCONV_FWD));
  else RD_TRY(launch_conv(h, h->plans[pls], h->d_plans + pls, B, s.hs[l - 1], h->fU[l], h->gch[l], h->fgS, et, st, RDGAN_TAG_GCONV_FWD));
  const bool fuse = a16 ? conv16_rows_owned(h->plans[ple]) : conv_rows_owned(h->plans[ple], B);
  RdEpi ep = epi_make(fuse ? RD_EPI_BIAS_PN_LRELU : RD_EPI_BIAS, gp + h->goff[2 * l + 1]);
  ep.rinv = s.rs[l];
  ep.addt = h->fgS; ep.addt_plane = 4 * sd[1] * sd[2] * h->gch[l];
  ep.nametag = l == 3;
  ep.out16 = a16;
  if (a16) RD_TRY(launch_conv16(h, h->plans[ple], h->d_plans + ple, B, h->fE[l], h->bU[l], s.hs[l], ep, st, tag));
  else RD_TRY(launch_conv(h, h->plans[ple], h->d_plans + ple, B, h->fE[l], h->fU[l], h->gch[l], s.hs[l], ep, st, tag));
  if (!fuse) {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    RD_TRY(launch_pn_fwd(h, s.hs[l], s.hs[l], s.rs[l], (long)B * h->gpix[l], h->gch[l], st, a16));
  }
  return 0;
}

// block l: UpSampling3D + Conv3D + bias (T:330-331), then PixelNorm + LeakyReLU (T:332-333).  keep_h3: see gen_forward_impl
static int gen_block_fwd(rdgan_handle* h, const GenPass& s, const float* gp, int l, int B, bool keep_h3, bool wait_forms, hipStream_t st) {
  const bool a16 = s.a16;
  float* const* hs = s.hs;
  float* const* rs = s.rs;
  const float* bias = gp + h->goff[2 * l + 1];
  const int tag = l == 3 ? RDGAN_TAG_GCONV3_FWD : RDGAN_TAG_GCONV_FWD;
  if (wait_forms) RD_CHECK(h, hipStreamWaitEvent(st, h->ev_g[l], 0));       // this block's weight forms
  if (gen_block_fast(h, l, fast_fwd_on(h))) return gen_block_fwd_shared_centre(h, s, gp, l, B, st);
  const float* Wl = gp + h->goff[2 * l];
  int pl = PL_G1F + l - 1;
  if (h->collapse) {
    Wl = h->GWC[l];
    pl = PL_G1FC + l - 1;
    if (!upconv_slab_on(h, l) && !upconv2_slab_on(h, l) && !upconv_slab_t_on(h, l)) pl = gen_box_plan(h, pl, PL_G1FCX + l - 1, B);
  }
  if (upconv_slab_on(h, l)) {     // block 3, bf16 storage: source slab resident in LDS, weights streamed in fragment order
    // (with the fused last conv the launch also carries that layer's 2 * rows * 64 * 27 FLOPs, and its tap products (Q12 in P9)
    // leave the kernel from the rows while they are in registers)
    const bool g9 = g9_fused_on(h);
    const double fl3 = plan_flops(h->plans[pl], B) + (g9 ? 2.0 * B * h->gpix[3] * 64 * 27 : 0.0);
    return launch_upconv_slab<1>(h, {pl, fl3, RDGAN_TAG_GCONV3_FWD}, hs[l - 1], h->bW3I, bias, hs[l], rs[l], B, nullptr,
                                 g9 ? h->bW9I : nullptr, g9 ? h->P9 : nullptr, keep_h3, st);
  }
  if (upconv_slab_t_on(h, l)) {   // block 3, bf16 storage, planes larger than 8 x 8: (h, w) tiles with their halo resident, K in two halves
    const bool g9t = g9_fused_t_on(h);
    const double fl3 = plan_flops(h->plans[pl], B) + (g9t ? 2.0 * B * h->gpix[3] * 64 * 27 : 0.0);
    return launch_upconv_slab_t(h, {pl, fl3, RDGAN_TAG_GCONV3_FWD}, hs[l - 1], h->bW3T, bias, hs[l], rs[l], B, h->gdim[2][1], h->gdim[2][2],
                                nullptr, g9t ? h->bW9I : nullptr, g9t ? h->P9 : nullptr, keep_h3, st);
  }
  if (upconv2_slab_on(h, l))      // block 2, bf16 storage: a sample resident in LDS, the four waves split the 128 channels
    return launch_upconv2_slab(h, {pl, plan_flops(h->plans[pl], B), RDGAN_TAG_GCONV_FWD}, hs[l - 1], h->bW2I, bias, hs[l], rs[l], B, st);
  const bool fuse = a16 ? conv16_rows_owned(h->plans[pl]) : conv_rows_owned(h->plans[pl], B);       // PixelNorm+LeakyReLU in the GEMM epilogue
  RdEpi ep = epi_make(fuse ? RD_EPI_BIAS_PN_LRELU : RD_EPI_BIAS, bias);
  ep.rinv = rs[l];
  ep.out16 = a16;
  ep.nametag = a16 && l == 3;
  if (a16)       // collapsed form (64 taps) on the bf16 matrix pipe
    RD_TRY(launch_conv16(h, h->plans[pl], h->d_plans + pl, B, hs[l - 1], h->bG1F[l], hs[l], ep, st, tag, h->conv_f16 ? h->fG1F[l] : nullptr));
  else RD_TRY(launch_conv(h, h->plans[pl], h->d_plans + pl, B, hs[l - 1], Wl, h->gch[l], hs[l], ep, st, tag));
  if (!fuse) {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    RD_TRY(launch_pn_fwd(h, hs[l], hs[l], rs[l], (long)B * h->gpix[l], h->gch[l], st, a16));
  }
  return 0;
}

// Conv3D 64->1 (T:345) as column GEMM + gather, bias, Softmax(axis=1) (T:347), check_numerics (T:349-350).
// When a 256-row tile holds whole (h,w) planes (nd = 8, 16) or whole w rows (nd = 32, 64, 128) the GEMM's epilogue
// sums the in-tile taps itself and writes 3 (9) floats per grid point instead of 32.
static int gen_last_conv_fwd(rdgan_handle* h, const GenPass& s, const float* gp, float* out, int B, hipStream_t st) {
  const int nd = h->nd;
  const bool a16 = s.a16;
  const int gq = 256 % (nd * nd) == 0 ? 3 : (256 % nd == 0 ? 9 : 0);
  const long ncol = (long)B * nd * nd;
  const long rows9 = (long)B * h->gpix[3];
  if (g9_fused_on(h)) {
    // the tap products left the block-3 slab kernel as Q12: the sums over kd and the source classes, bias, softmax
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_tapsum_softmax12(h->P9, gp + h->goff[9], out, B, h->d_flag, st);
  } else if (g9_fused_t_on(h)) {
    // the same behind the tiled kernel: main sums per tile + the halo terms of the neighbouring tiles
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    const int TH = h->gdim[2][1] / 8, TW = h->gdim[2][2] / 8;
    const long nthr = (long)B * 6 * TH * TW * 24 * 32;
    hipLaunchKernelGGL(k_g9_halo_fold, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, h->P9, B, TH, TW);
    hipLaunchKernelGGL((k_tapsum_softmax12t<RDGAN_NHOURS>), dim3((unsigned)((ncol / 4 + 63) / 64)), dim3(256), 0, st, h->P9,
                       gp + h->goff[9], out, B, h->gdim[2][1], h->gdim[2][2], h->d_flag);
  } else if (!a16 && h->tapgather && h->edge_kernels == 1 && g9w_mfma_ok(nd, rows9)) {
    // fp32 storage: pipelined streaming kernel on 128-pixel tiles (rdgan_edge.hip.h), nine kw-sums per grid point
    ProfScope ps(h, RDGAN_TAG_GCONV_FWD, st);
    LaunchScope ls(h, PL_G9F, RD_KIND_EDGE, B, 2.0 * rows9 * 64 * 27, st);
    RD_KNAME(h, "k_g9_fwd_mfma + k_tapsum_softmax");
    h->flops_acc += 2.0 * rows9 * 64 * 27;
    if (nd * nd <= 256) {       // whole (h,w) planes in a 256-pixel tile: three sums per grid point
      const size_t lds9 = (size_t)(256 * 64 + 256 * 33) * sizeof(float);
      RD_TRY(ensure_lds(h, (const void*)k_g9_fwd_mfma<256>, lds9));
      hipLaunchKernelGGL(k_g9_fwd_mfma<256>, dim3((unsigned)std::min<long>((rows9 + 255) / 256, 256)), dim3(512), lds9, st,
                         (const float*)h->h3, gp + h->goff[8], h->P9, rows9, nd, 2 * ilog2(nd));
      launch_tapsum_softmax(h, 3, out, gp, B, st);
    } else {
      const size_t lds9 = (size_t)(128 * 64 + 128 * 33) * sizeof(float);
      RD_TRY(ensure_lds(h, (const void*)k_g9_fwd_mfma<128>, lds9));
      hipLaunchKernelGGL(k_g9_fwd_mfma<128>, dim3((unsigned)std::min<long>((rows9 + 127) / 128, 768)), dim3(256), lds9, st,
                         (const float*)h->h3, gp + h->goff[8], h->P9, rows9, nd, 2 * ilog2(nd));
      launch_tapsum_softmax(h, 9, out, gp, B, st);
    }
  } else if (gq && h->tapgather && (h->edge_kernels >= 2 || (h->edge_kernels && a16))) {
    // dedicated streaming kernel (rdgan_edge.hip.h): same tiles, same arithmetic and output as the tap-gathering GEMM below.
    // Default in the bf16 storage mode (one pass over h3 at 5.4 TB/s: 37 us against 153 us at bs 256); with fp32 storage its
    // one-tile-per-workgroup form (64 KB tiles, two workgroups per CU in lockstep) only matches the GEMM (159 vs 147 us),
    // so fp32 keeps the GEMM unless "edge_kernels" is 2 (tests).
    ProfScope ps(h, RDGAN_TAG_GCONV_FWD, st);
    LaunchScope ls(h, PL_G9F, RD_KIND_EDGE, B, 2.0 * rows9 * 64 * 27, st);
    RD_KNAME(h, "k_g9_fwd + k_tapsum_softmax");
    h->flops_acc += 2.0 * rows9 * 64 * 27;
    RD_TRY(ensure_lds(h, a16 ? (const void*)k_g9_fwd<rd_bf16_t> : (const void*)k_g9_fwd<float>, a16 ? 36 * 1024 : 72 * 1024));
    const dim3 g9((unsigned)((rows9 + 255) / 256));
    if (a16) hipLaunchKernelGGL(k_g9_fwd<rd_bf16_t>, g9, dim3(256), 36 * 1024, st, (const rd_bf16_t*)h->h3, gp + h->goff[8], h->P9, rows9, nd, nd * nd, gq);
    else hipLaunchKernelGGL(k_g9_fwd<float>, g9, dim3(256), 72 * 1024, st, (const float*)h->h3, gp + h->goff[8], h->P9, rows9, nd, nd * nd, gq);
    launch_tapsum_softmax(h, gq, out, gp, B, st);
  } else if (gq && h->tapgather) {
    RdEpi e = epi_make(RD_EPI_TAPGATHER);
    e.gw = nd; e.ghw = nd * nd; e.gq = gq;
    if (a16) RD_TRY(launch_conv_a16(h, h->plans[PL_G9F], h->d_plans + PL_G9F, B, h->h3, h->W9T, 32, h->P9, e, st, -1, true, false));
    else RD_TRY(launch_conv(h, h->plans[PL_G9F], h->d_plans + PL_G9F, B, h->h3, h->W9T, 32, h->P9, e, st, -1));
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_tapsum_softmax(h, gq, out, gp, B, st);
  } else {
    const RdEpi e = epi_make(RD_EPI_PLAIN);
    if (a16) RD_TRY(launch_conv_a16(h, h->plans[PL_G9F], h->d_plans + PL_G9F, B, h->h3, h->W9T, 32, h->P9, e, st, -1, true, false));
    else RD_TRY(launch_conv(h, h->plans[PL_G9F], h->d_plans + PL_G9F, B, h->h3, h->W9T, 32, h->P9, e, st, -1));
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_colgather_softmax(h->P9, gp + h->goff[9], out, B, nd, nd, h->d_flag, st);
  }
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// keep_h3: block 3's output and 1/l2 are needed afterwards (generator step: its backward; rdgan_gen_forward: the test hook) --
// a critic step passes false, and with the fused last conv the 1.6 GB tensor (2048 samples) is then never written
// `ws`: stream of the weight-only kernels (the handle's side stream, forked by the caller, or `st` itself): the weight forms of
// block l are complete behind event ev_g[l], which `st` waits for in front of the block's GEMM
static int gen_forward_impl(rdgan_handle* h, const float* gp, const float* z, const float* cond, float* out, int B,
                            hipStream_t st, hipStream_t ws, bool keep_h3 = true) {
  RD_TRY(a16_check(h));
  const GenPass s = gen_pass(h, B);
  bool built = false;
  RD_TRY(gen_build_forms(h, gp, st, ws, &built));
  const bool wait_forms = built && ws != st;
  RD_TRY(gen_dense_fwd(h, s, gp, z, cond, B, wait_forms, st));
  for (int l = 1; l <= 3; ++l) RD_TRY(gen_block_fwd(h, s, gp, l, B, keep_h3, wait_forms, st));
  return gen_last_conv_fwd(h, s, gp, out, B, st);
}

static bool fwd_ahead_on(const rdgan_handle* h) { return h->ahead && h->ev_ahead_done && (h->fwd_ahead < 0 ? !h->a16 : h->fwd_ahead); }

// `st` waits for an early generator forward still in flight, which is then dropped: every entry that uses the workspace
// calls this first, except the generator step that consumes the forward
static int ahead_drain(rdgan_handle* h, hipStream_t st) {
  if (!h->ahead_pending) return 0;
  h->ahead_pending = false;
  RD_CHECK(h, hipStreamWaitEvent(st, h->ev_ahead_done, 0));
  return 0;
}

// the early generator forward (see the handle): forked from `st` behind everything issued there so far, on the handle's own
// stream, with its own split-K slab and non-finite flag.  The arithmetic is that of the forward in rdgan_gen_grad_after.
static int ahead_issue(rdgan_handle* h, const float* gp, const float* z, const float* cond, int B, hipStream_t st) {
  RD_CHECK(h, hipEventRecord(h->ev_ahead_fork, st));
  RD_CHECK(h, hipStreamWaitEvent(h->ahead, h->ev_ahead_fork, 0));
  std::swap(h->kpartial, h->kpartial_ahead);
  std::swap(h->d_flag, h->flag_ahead);
  const int rc = gen_forward_impl(h, gp, z, cond, h->fake, B, h->ahead, h->ahead);
  std::swap(h->kpartial, h->kpartial_ahead);
  std::swap(h->d_flag, h->flag_ahead);
  RD_TRY(rc);
  RD_CHECK(h, hipEventRecord(h->ev_ahead_done, h->ahead));
  h->ahead_pending = true;
  h->ahead_gp = gp; h->ahead_z = z; h->ahead_cond = cond; h->ahead_B = B; h->ahead_gver = h->gver_in;
  return 0;
}

extern "C" int rdgan_gen_forward(rdgan_handle* h, const float* gen_params, const float* z, const float* cond,
                                 float* out, int B, void* stream) {
  if (!h || !gen_params || !z || !cond || !out) return bad_arg(h, "gen_forward: null pointer");
  if (B < 1 || B > h->MB) return bad_arg(h, "gen_forward: B outside [1, max_batch]");
  RD_TRY(ahead_drain(h, (hipStream_t)stream));
  return gen_forward_impl(h, gen_params, z, cond, out, B, (hipStream_t)stream, side_fork(h, (hipStream_t)stream));
}

// tf.debugging.check_numerics behind the generator's softmax (T:349-350): the softmax kernels raise a device flag on
// NaN/Inf; this waits for `stream` and reports the flag of the calls issued since the last reset (every public
// generator-forward / gradient entry resets it first).
extern "C" int rdgan_check_numerics(rdgan_handle* h, void* stream) {
  if (!h) return -2;
  RD_CHECK(h, hipStreamSynchronize((hipStream_t)stream));
  int flag = 0;
  RD_CHECK(h, hipMemcpy(&flag, h->d_flag, sizeof(int), hipMemcpyDeviceToHost));
  if (flag) { h->err = "check_numerics: the generator output contains NaN or Inf"; return -1; }
  return 0;
}

// ------------------------------------------------------------------------------------
// critic
// ------------------------------------------------------------------------------------
static bool d2_slab_on(const rdgan_handle* h) { return h->d2_slab && h->a16 && h->nd == 16; }
// the same on tiles of 8 x 8 destination positions (k_d2_dgrad_slab_t16): ndomain 32, 48, 64, ... (layer 2's output grid a multiple of 4 x 4)
static bool d2_slab_t_on(const rdgan_handle* h) {
  return h->d2_slab && h->a16 && h->nd > 16 && h->nd % 16 == 0 && h->ddim[2][1] % 4 == 0 && h->ddim[2][2] % 4 == 0 && h->ddim[2][0] == 6 &&
         h->ddim[1][1] == 2 * h->ddim[2][1] - 1 && h->ddim[1][2] == 2 * h->ddim[2][2] - 1 && h->dpad[1][0] == 1 && h->dpad[1][1] == 1 && h->dpad[1][2] == 1;
}
static bool d2_fwd_slab_on(const rdgan_handle* h) { return h->d2_fwd_slab && h->a16 && h->nd == 16; }
static int prep_critic_weights(rdgan_handle* h, const float* dp, hipStream_t st) {
  // (skipped when the forms in the workspace were built from these very weights: see rdgan_set_weight_versions)
  const int ccfg = rd_form_key(h, RD_FORMS_CRITIC);    // every option this function reads, directly or through a predicate
  if (h->cver_in != 0 && dp == h->ccache_ptr && h->cver_in == h->ccache_ver && ccfg == h->ccache_cfg) return 0;
  h->form_builds[1]++;
  h->ccache_ptr = nullptr; h->ccache_ver = 0; h->ccache_cfg = -1;     // (valid again only once every form kernel has been issued)
  if (!h->a16) {       // fp32 storage: transposed kernels of the input-gradient GEMMs (the bf16 storage mode reads bf16 images instead)
    for (int l = 2; l <= 4; ++l)   // [27][Cin][Cout] -> [27][Cout][Cin]
      RD_TRY(launch_transpose(h, dp + h->doff[2 * (l - 1)], h->DWT[l], 27, h->dch[l - 1], h->dch[l], h->dch[l - 1], st));
    // W1 [27*Cin][64] -> W1T [64][ldp1] (columns (tap,ci), zero padded)
    RD_TRY(launch_transpose(h, dp + h->doff[0], h->W1T, 1, 27 * h->Cin, 64, h->ldp1, st));
  }
  if (h->CP != h->Cin) hipLaunchKernelGGL(k_pad_w1, dim3(27), dim3(256), 0, st, dp + h->doff[0], h->W1P, h->Cin, h->CP);
  if (h->a16) {
    // layers 2-4 in ONE launch per image kind (forward [27][Cout][Cin], input gradient [27][Cin][Cout]): 3 launches per build
    // instead of 11 -- the critic's forms are rebuilt after each of its n_critic updates per iteration
    RdW3 a;
    for (int l = 2; l <= 4; ++l) {
      a.in[l - 2] = dp + h->doff[2 * (l - 1)];
      a.outT[l - 2] = (unsigned short*)h->bWF[l]; a.outC[l - 2] = (unsigned short*)h->bWB[l];
      a.outTf[l - 2] = h->conv_f16 ? (unsigned short*)h->fWF[l] : nullptr; a.outCf[l - 2] = h->conv_f16 ? (unsigned short*)h->fWB[l] : nullptr;
      a.K[l - 2] = h->dch[l - 1]; a.N[l - 2] = h->dch[l];
    }
    hipLaunchKernelGGL(k_weights3_to_bf16, dim3(8, 8, 3 * 27), dim3(256), 0, st, a);
    if (d2_fwd_slab_on(h))
      launch_d2f_wimg(dp + h->doff[2], h->bW2F, st);
    if (d2_slab_on(h) || d2_slab_t_on(h)) launch_d2s_wimg(dp + h->doff[2], h->bW2S, st);
    hipLaunchKernelGGL(k_w1_to_bf16, dim3(ew_blocks(64L * h->ldp1)), dim3(256), 0, st, dp + h->doff[0], (rd_bf16_t*)h->bW1B,
                       27 * h->Cin, h->ldp1);
  }
  RD_CHECK(h, hipGetLastError());
  h->ccache_ptr = dp; h->ccache_ver = h->cver_in; h->ccache_cfg = ccfg;
  return 0;
}

// D1's forward weights: the caller's [27][Cin][64] kernel, or its zero-padded [27][CP][64] copy when CP > Cin
static inline const float* d1_weights(const rdgan_handle* h, const float* dp) {
  return h->CP != h->Cin ? h->W1P : dp + h->doff[0];
}

// First critic layer as one K = 64 GEMM per tile (rdgan_edge.hip.h): one condition channel (2 floats per voxel), any ndomain
static bool d1_gemm_ok(const rdgan_handle* h) { return h->edge_kernels && h->CP == 2 && h->Cin == 2; }
// critic layer 2's weight gradient by k_d2_wgrad_slab16 (bf16 storage mode, ndomain 16): a wave owns one tap, its [64 x 128]
// product stays in registers over the workgroup's share of the batch
static bool d2_wgrad_slab_on(const rdgan_handle* h) { return h->a16 && h->d2_wgrad_slab && h->nd == 16; }
// layer 3's by k_d3_wgrad_slab16: a wave owns (tap, quarter of the output channels); items of four samples (12 output positions each)
static bool d3_wgrad_slab_on(const rdgan_handle* h) { return h->a16 && h->d3_wgrad_slab && h->nd == 16; }
// layer 2's on tiles of 4 x 4 output positions (k_d2_wgrad_slab_t16; ndomain 32 / 48 / 64): the geometry of 'valid' layer 1 +
// stride-2 'same' layer 2 on an ndomain that is a multiple of 16 (11 x (2 OH - 1)^2 -> 6 x OH^2, OH % 4 == 0)
static bool d2_wgrad_slab_t_on(const rdgan_handle* h) {
  return h->d2_wgrad_slab && h->a16 && h->nd > 16 && h->nd % 16 == 0 && h->ddim[1][0] == 11 && h->ddim[2][0] == 6 &&
         h->ddim[2][1] % 4 == 0 && h->ddim[2][2] % 4 == 0 && h->ddim[1][1] == 2 * h->ddim[2][1] - 1 && h->ddim[1][2] == 2 * h->ddim[2][2] - 1 &&
         h->dch[1] == 64 && h->dch[2] == 128;
}
static bool d2_gate_bits_on(const rdgan_handle* h) {
  return h->d2_gate_bits && h->d2_slab && h->a16 && (h->nd == 16 || d2_slab_t_on(h)) && h->g1bits;
}
static int launch_d1_fwd(rdgan_handle* h, const float* in, const float* w, const float* bias, float* out, const float* aux, int NBt,
                         int mode, int use_drop, uint32_t key, uint32_t idx_base, hipStream_t st) {
  unsigned char* gbits = mode == 0 && d2_gate_bits_on(h) ? h->g1bits : nullptr;
  ProfScope ps(h, RDGAN_TAG_CRITIC_GEMM, st);
  const long rows = (long)NBt * h->dL[1];
  LaunchScope ls(h, PL_D1F, RD_KIND_EDGE, NBt, 2.0 * rows * 54 * 64, st);
  if (h->d1_fwd_sample && h->a16 && h->nd == 16 && h->CP == 2 && h->dL[1] == RD_D1S_NPOS && (mode == 0 || d2_gate_bits_on(h))) {
    // a sample's input volume resident in LDS (rdgan_d1fwd16.hip.h).  Mode 1 (second sweep, in place over the x_hat third) takes the
    // gate from the 2-bit codes the forward left for the rows at element offset idx_base
    RD_KNAME(h, "k_d1_fwd_sample16<bf16,%d>", mode);
    h->flops_acc += 2.0 * rows * 54 * 64;
    const dim3 grid((unsigned)std::min(NBt, 768));
    if (mode == 0) {
      RD_TRY(ensure_lds(h, (const void*)k_d1_fwd_sample16<0>, RD_D1S_LDS));
      hipLaunchKernelGGL(k_d1_fwd_sample16<0>, grid, dim3(256), RD_D1S_LDS, st, in, w, bias, (rd_bf16_t*)out, gbits, NBt, use_drop, key, idx_base);
    } else {
      RD_TRY(ensure_lds(h, (const void*)k_d1_fwd_sample16<1>, RD_D1S_LDS));
      hipLaunchKernelGGL(k_d1_fwd_sample16<1>, grid, dim3(256), RD_D1S_LDS, st, in, w, bias, (rd_bf16_t*)out,
                         h->g1bits + (size_t)(idx_base / 64) * 16, NBt, use_drop, key, idx_base);
    }
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  RD_KNAME(h, "k_d1_gemm_fwd<%s,%d>", h->a16 ? "bf16" : "f32", mode);
  h->flops_acc += 2.0 * rows * 54 * 64;
  constexpr size_t lds = (size_t)(128 * 64 + 64 * 64) * 4 + 2 * 128 * 8;
  const dim3 grid((unsigned)std::min<long>((rows + 127) / 128, 768));       // three workgroups per CU, each walks its tiles
  const int nd = h->nd, Do = h->ddim[1][0], Ho = h->ddim[1][1], Wo = h->ddim[1][2];
#define RD_D1F(TO, MODE)                                                                                                   \
  do {                                                                                                                     \
    RD_TRY(ensure_lds(h, (const void*)k_d1_gemm_fwd<TO, MODE>, lds));                                                      \
    hipLaunchKernelGGL((k_d1_gemm_fwd<TO, MODE>), grid, dim3(256), lds, st, in, w, bias, (TO*)out, (const TO*)aux, rows, nd, \
                       Do, Ho, Wo, use_drop, key, idx_base, gbits);                                                        \
  } while (0)
  if (h->a16) { if (mode == 0) RD_D1F(rd_bf16_t, 0); else RD_D1F(rd_bf16_t, 1); }
  else { if (mode == 0) RD_D1F(float, 0); else RD_D1F(float, 1); }
#undef RD_D1F
  RD_CHECK(h, hipGetLastError());
  return 0;
}
// bf16 storage mode: the layer-1 weight gradient on the bf16 matrix pipe, bias gradient (rows < bias_rows) in the same pass
static bool d1_wgrad16_on(const rdgan_handle* h) { return h->a16 && h->d1_wgrad16; }
static int launch_d1_wgrad(rdgan_handle* h, const float* in, const float* u1, float* dW, int NBt, hipStream_t st,
                           float* db = nullptr, long bias_rows = 0) {
  ProfScope ps(h, RDGAN_TAG_CRITIC_GEMM, st);
  const long rows = (long)NBt * h->dL[1];
  if (d1_wgrad16_on(h)) {
    LaunchScope ls(h, PL_D1F, RD_KIND_WGRAD, NBt, 2.0 * rows * 54 * 64, st);
    RD_KNAME(h, "k_d1_wgrad16<bf16>");
    h->flops_acc += 2.0 * rows * 54 * 64;
    long G = std::min<long>(1024, (rows + 63) / 64);
    long rpw = ((rows + G - 1) / G + 63) / 64 * 64;
    G = (rows + rpw - 1) / rpw;
    if ((size_t)G * 4096 > h->wpartial_cap) return bad_arg(h, "d1 wgrad: partial workspace too small");
    hipLaunchKernelGGL(k_d1_wgrad16, dim3((unsigned)G), dim3(256), 0, st, in, (const rd_bf16_t*)u1, h->wpartial, rows, rpw,
                       db ? bias_rows : 0L, h->nd, h->ddim[1][0], h->ddim[1][1], h->ddim[1][2]);
    hipLaunchKernelGGL(k_d1_wgrad_fold, dim3((db ? 55 : 54) * 64 / 16), dim3(256), 0, st, h->wpartial, (int)G, dW, db);
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  LaunchScope ls(h, PL_D1F, RD_KIND_WGRAD, NBt, 2.0 * rows * 54 * 64, st);
  RD_KNAME(h, "k_d1_gemm_wgrad<%s>", h->a16 ? "bf16" : "f32");
  h->flops_acc += 2.0 * rows * 54 * 64;
  // one slice of rows per workgroup: four workgroups per CU, whole 32-row chunks
  long G = std::min<long>(1024, (rows + 31) / 32);
  long rpw = ((rows + G - 1) / G + 31) / 32 * 32;
  G = (rows + rpw - 1) / rpw;
  if ((size_t)G * 4096 > h->wpartial_cap) return bad_arg(h, "d1 wgrad: partial workspace too small");
  const int nd = h->nd, Do = h->ddim[1][0], Ho = h->ddim[1][1], Wo = h->ddim[1][2];
  if (h->a16) hipLaunchKernelGGL(k_d1_gemm_wgrad<rd_bf16_t>, dim3((unsigned)G), dim3(256), 0, st, in, (const rd_bf16_t*)u1, h->wpartial, rows,
                                 rpw, nd, Do, Ho, Wo);
  else hipLaunchKernelGGL(k_d1_gemm_wgrad<float>, dim3((unsigned)G), dim3(256), 0, st, in, u1, h->wpartial, rows, rpw, nd, Do, Ho, Wo);
  hipLaunchKernelGGL(k_d1_wgrad_fold, dim3(54 * 64 / 16), dim3(256), 0, st, h->wpartial, (int)G, dW);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// forward over NBt samples already laid out in h->cin; writes h->dh[1..4], h->v
static int critic_forward_impl(rdgan_handle* h, const float* dp, int NBt, uint64_t seed, hipStream_t st) {
  const int use_drop = seed != 0;
  const bool a16 = h->a16 != 0;
  const float* in = h->cin;
  for (int l = 1; l <= 4; ++l) {
    int pl = l == 1 ? PL_D1F : critic_fwd_plan(h, l, NBt);
    RdEpi ep = epi_make(RD_EPI_BIAS_LRELU_DROP, dp + h->doff[2 * (l - 1) + 1], nullptr, use_drop,
                        rd_make_key(seed, RD_STREAM_D1 + l - 1), 0);
    ep.out16 = a16;
    if (l == 1 && d1_gemm_ok(h))
      RD_TRY(launch_d1_fwd(h, in, dp + h->doff[0], dp + h->doff[1], h->dh[1], nullptr, NBt, 0, use_drop, ep.key, 0, st));
    else if (a16 && l == 1)
      RD_TRY(launch_conv_a16(h, h->plans[pl], h->d_plans + pl, NBt, in, d1_weights(h, dp), h->dch[l], h->dh[l], ep, st,
                             RDGAN_TAG_CRITIC_GEMM, false, true));
    else if (l == 2 && d2_fwd_slab_on(h))      // a sample's layer-1 output resident in LDS, the four waves split the 128 channels
      RD_TRY(launch_d2_fwd_slab(h, {pl, plan_flops(h->plans[pl], NBt), RDGAN_TAG_CRITIC_GEMM}, in, h->bW2F, dp + h->doff[3], h->dh[2], NBt,
                                use_drop, ep.key, st));
    else if (a16)
      RD_TRY(launch_conv16(h, h->plans[pl], h->d_plans + pl, NBt, in, h->bWF[l], h->dh[l], ep, st, RDGAN_TAG_CRITIC_GEMM,
                           h->conv_f16 ? h->fWF[l] : nullptr));
    else
    RD_TRY(launch_conv(h, h->plans[pl], h->d_plans + pl, NBt, in, l == 1 ? d1_weights(h, dp) : dp + h->doff[2 * (l - 1)],
                       h->dch[l], h->dh[l], ep, st, RDGAN_TAG_CRITIC_GEMM));
    in = h->dh[l];
  }
  ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
  launch_critic_dense_fwd(a16, h->dh[4], dp + h->doff[8], dp + h->doff[9], h->v, NBt, h->F, st);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// input-gradient chain u4 -> u1 over NBt samples (mode 0: critic step 3B batch, 1: generator step)
static int critic_dgrad_chain(rdgan_handle* h, const float* dp, int NBt, int B, int mode, uint64_t seed, hipStream_t st) {
  const int use_drop = seed != 0;
  const bool a16 = h->a16 != 0;
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_critic_top_bwd(a16, h->dh[4], dp + h->doff[8], h->du[4], NBt, h->F, B, mode, seed, st);
  }
  for (int l = 4; l >= 2; --l) {
    int pl = critic_dgrad_plan(h, l, NBt);
    RdEpi ep = epi_make(RD_EPI_GATE_AUX, nullptr, h->dh[l - 1], use_drop, rd_make_key(seed, RD_STREAM_D1 + l - 2), 0);
    ep.out16 = a16;
    const unsigned char* gbits = d2_gate_bits_on(h) && d1_gemm_ok(h) ? h->g1bits : nullptr;
    if (l == 2 && d2_slab_on(h)) {      // two samples' output gradient resident in LDS, weights streamed in fragment order
      RD_TRY(launch_d2_dgrad_slab(h, {pl, plan_flops(h->plans[pl], NBt), RDGAN_TAG_CRITIC_GEMM}, h->du[2], h->bW2S, h->dh[1], h->du[1], NBt,
                                  use_drop, gbits, st));
      continue;
    }
    if (l == 2 && d2_slab_t_on(h)) {    // the same on tiles: two samples' 6 x 5 x 5 output-gradient positions per tile resident
      const int one = PL_D2B;               // (FLOPs of the one-phase plan: the slab kernel multiplies every (position, tap) pair that lands inside)
      RD_TRY(launch_d2_dgrad_slab_t(h, {one, plan_flops(h->plans[one], NBt), RDGAN_TAG_CRITIC_GEMM}, h->du[2], h->bW2S, h->dh[1], h->du[1], NBt,
                                    h->ddim[2][1], h->ddim[2][2], use_drop, gbits, st));
      continue;
    }
    if (a16)
      RD_TRY(launch_conv16(h, h->plans[pl], h->d_plans + pl, NBt, h->du[l], h->bWB[l], h->du[l - 1], ep, st, RDGAN_TAG_CRITIC_GEMM,
                           h->conv_f16 ? h->fWB[l] : nullptr));
    else
    RD_TRY(launch_conv(h, h->plans[pl], h->d_plans + pl, NBt, h->du[l], h->DWT[l], h->dch[l - 1], h->du[l - 1], ep, st,
                       RDGAN_TAG_CRITIC_GEMM));
  }
  return 0;
}

// dD/d(sample channel) for `B` samples whose u1 starts at u1: column GEMM + col2im -> h->g0
// cin_hat (the gradient-penalty sweep): where the one-pass fp32 kernel runs it also leaves the penalty's norm, coefficient and
// second-sweep input (k_gp_norm_r0's outputs: h->gpv, cin_hat) and sets *norm_done; otherwise the caller launches that pass
static int critic_input_grad(rdgan_handle* h, const float* dp, const float* u1, int B, hipStream_t st, float* cin_hat = nullptr,
                             bool* norm_done = nullptr) {
  if (norm_done) *norm_done = false;
  if (!h->a16 && h->d1_dgrad_fused && h->nd == 16 && d1_gemm_ok(h)) {     // one pass, no column matrix (k_d1_dgrad_sample32)
    ProfScope ps(h, RDGAN_TAG_CRITIC_GEMM, st);
    LaunchScope ls(h, PL_D1B, RD_KIND_CONV, B, 2.0 * B * h->dL[1] * 27 * 64, st);
    h->flops_acc += 2.0 * B * h->dL[1] * 27 * 64;
    const dim3 grid((unsigned)std::min(B, 512));
    if (cin_hat && norm_done) {
      RD_KNAME(h, "k_d1_dgrad_sample32<gp>");
      RD_TRY(ensure_lds(h, (const void*)k_d1_dgrad_sample32<true>, RD_D1DG_LDS_GP));
      hipLaunchKernelGGL(k_d1_dgrad_sample32<true>, grid, dim3(256), RD_D1DG_LDS_GP, st, u1, dp + h->doff[0], h->g0, B, cin_hat, h->gpv,
                         RD_GP_WEIGHT);
      *norm_done = true;
    } else {
      RD_KNAME(h, "k_d1_dgrad_sample32");
      RD_TRY(ensure_lds(h, (const void*)k_d1_dgrad_sample32<false>, RD_D1DG_LDS));
      hipLaunchKernelGGL(k_d1_dgrad_sample32<false>, grid, dim3(256), RD_D1DG_LDS, st, u1, dp + h->doff[0], h->g0, B, (float*)nullptr,
                         (float*)nullptr, 0.f);
    }
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  if (h->a16 && h->d1_dgrad_fused && h->nd == 16 && d1_gemm_ok(h)) {      // one pass, no column matrix (k_d1_dgrad_sample16)
    ProfScope ps(h, RDGAN_TAG_CRITIC_GEMM, st);
    LaunchScope ls(h, PL_D1B, RD_KIND_CONV, B, 2.0 * B * h->dL[1] * 27 * 64, st);
    RD_KNAME(h, "k_d1_dgrad_sample16<bf16>");
    h->flops_acc += 2.0 * B * h->dL[1] * 27 * 64;
    RD_TRY(ensure_lds(h, (const void*)k_d1_dgrad_sample16, RD_D1DG_LDS));
    hipLaunchKernelGGL(k_d1_dgrad_sample16, dim3((unsigned)std::min(B, 512)), dim3(256), RD_D1DG_LDS, st, (const rd_bf16_t*)u1,
                       dp + h->doff[0], h->g0, B);
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  if (h->a16 && h->d1_dgrad_fused && h->nd > 16 && h->nd % 16 == 0 && d1_gemm_ok(h)) {      // the same on 24 x 16 x 8 input tiles (k_d1_dgrad_tile16)
    ProfScope ps(h, RDGAN_TAG_CRITIC_GEMM, st);
    LaunchScope ls(h, PL_D1B, RD_KIND_CONV, B, 2.0 * B * h->dL[1] * 27 * 64, st);
    RD_KNAME(h, "k_d1_dgrad_tile16<bf16>");
    h->flops_acc += 2.0 * B * h->dL[1] * 27 * 64;
    RD_TRY(ensure_lds(h, (const void*)k_d1_dgrad_tile16, RD_D1DT_LDS));
    const long items = (long)B * (h->nd / 16) * (h->nd / 8);
    hipLaunchKernelGGL(k_d1_dgrad_tile16, dim3((unsigned)std::min<long>(items, 1024)), dim3(256), RD_D1DT_LDS, st, (const rd_bf16_t*)u1,
                       dp + h->doff[0], h->g0, B, h->nd);
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  if (h->a16)     // bf16 u1 against the bf16 first kernel [ldp1][64], fp32 column matrix
    RD_TRY(launch_conv16(h, h->plans[PL_D1B], h->d_plans + PL_D1B, B, u1, h->bW1B, h->P1, epi_make(RD_EPI_PLAIN), st,
                         RDGAN_TAG_CRITIC_GEMM));
  else
  RD_TRY(launch_conv(h, h->plans[PL_D1B], h->d_plans + PL_D1B, B, u1, h->W1T, h->ldp1, h->P1, epi_make(RD_EPI_PLAIN), st,
                     RDGAN_TAG_CRITIC_GEMM));
  ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
  hipLaunchKernelGGL(k_d1_col2im, dim3(ew_blocks((long)B * h->dL[0])), dim3(256), 0, st, h->P1, h->g0, B, h->ddim[0][0],
                     h->ddim[0][1], h->ddim[0][2], h->ddim[1][0], h->ddim[1][1], h->ddim[1][2], h->Cin, h->ldp1);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// gradient penalty (T:238-241, T:382) from the x_hat third's u1: h->g0 = dD/dx_hat, h->gpv = ||g0|| - 1 per sample, cin_hat = the
// second sweep's input (r0, 0) -- in one pass where critic_input_grad has one, else the norm in a pass of its own
static int critic_penalty_input(rdgan_handle* h, const float* dp, const float* u1, int B, float* cin_hat, hipStream_t st) {
  bool norm_done = false;
  RD_TRY(critic_input_grad(h, dp, u1, B, st, cin_hat, &norm_done));
  if (norm_done) return 0;
  ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
  // S blocks per sample when there are few samples of many elements (ndomain 64)
  const int per = (int)h->dL[0];
  launch_gp_norm(h->g0, h->gp_part, cin_hat, h->gpv, per, B, h->CP, gp_norm_slices(B, per), st);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

extern "C" int rdgan_critic_forward(rdgan_handle* h, const float* critic_params, const float* sample, const float* cond,
                                    float* out, int B, uint64_t seed, void* stream) {
  if (!h || !critic_params || !sample || !cond || !out) return bad_arg(h, "critic_forward: null pointer");
  if (B < 1 || B > h->NB) return bad_arg(h, "critic_forward: B outside [1, 3*max_batch]");
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ahead_drain(h, st));
  h->gate_keep_B = 0;
  RD_TRY(a16_check(h));
  if (h->a16) RD_TRY(prep_critic_weights(h, critic_params, st));      // (also makes the bf16 kernels of layers 2-4)
  else if (h->CP != h->Cin && !(h->cver_in != 0 && critic_params == h->ccache_ptr && h->cver_in == h->ccache_ver)) {
    // fp32 storage only needs the padded layer-1 kernel here.  W1P now belongs to THESE weights: whatever forms were cached
    // (a trainer's critic on the shared engine, models.get_engine) no longer describe the workspace
    hipLaunchKernelGGL(k_pad_w1, dim3(27), dim3(256), 0, st, critic_params + h->doff[0], h->W1P, h->Cin, h->CP);
    h->ccache_ptr = nullptr; h->ccache_ver = 0; h->ccache_cfg = -1;
  }
  launch_build_critic_input(h, sample, nullptr, cond, B, 2, 0u, 0u, st);
  RD_TRY(critic_forward_impl(h, critic_params, B, seed, st));
  RD_CHECK(h, hipMemcpyAsync(out, h->v, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
  return 0;
}

// ---- stages of the critic step behind its forward and input-gradient chain (rdgan_critic_grad_ahead)
// bias gradients: only the real|fake passes reach the loss through the bias (the penalty term does not).  Column sums of
// the output gradients the chain has just left: on the side stream, beside the penalty's second sweep and the weight-gradient
// GEMMs (nothing behind the chain writes du[l]; the column-sum scratch is used by these launches only)
static int critic_bias_grads(rdgan_handle* h, float* grad, int B, hipStream_t st) {
  hipStream_t cs = side_fork(h, st);
  for (int l = 1; l <= 4; ++l) {
    if (l == 1 && d1_gemm_ok(h) && d1_wgrad16_on(h)) continue;      // comes out of the weight-gradient GEMM (k_d1_wgrad16)
    RD_TRY(launch_colsum(h, h->du[l], (long)2 * B * h->dL[l], h->dch[l], grad + h->doff[2 * (l - 1) + 1], cs, h->a16 != 0));
  }
  return 0;
}

// second forward sweep of the double backward: r_l = gate_l * conv_l(r_{l-1}), in place over the x_hat third
static int critic_second_sweep(rdgan_handle* h, const float* dp, const float* cin_hat, int B, uint64_t seed, hipStream_t st) {
  const bool a16 = h->a16 != 0;
  const int use_drop = seed != 0;
  h->gate_keep_B = 0;
  if (h->keep_gates) {       // test hook: keep the x_hat third of every h_l (see rdgan_debug_activation)
    for (int l = 1; l <= 4; ++l) {
      const long third = (long)2 * B * h->dL[l] * h->dch[l];
      RD_CHECK(h, hipMemcpyAsync(h->gate_keep[l], act_off(h, h->dh[l], third), (size_t)(third / 2) * (a16 ? 2 : 4), hipMemcpyDeviceToDevice, st));
    }
    h->gate_keep_B = B;
  }
  const float* in = cin_hat;
  for (int l = 1; l <= 4; ++l) {
    int pl = l == 1 ? PL_D1F : critic_fwd_plan(h, l, B);
    long third = (long)2 * B * h->dL[l] * h->dch[l];
    float* dst = act_off(h, h->dh[l], third);
    RdEpi ep = epi_make(RD_EPI_GATE_AUX, nullptr, dst, use_drop, rd_make_key(seed, RD_STREAM_D1 + l - 1), (uint32_t)third);
    ep.out16 = a16;
    if (l == 1 && d1_gemm_ok(h)) RD_TRY(launch_d1_fwd(h, in, dp + h->doff[0], nullptr, dst, dst, B, 1, use_drop, ep.key, (uint32_t)third, st));
    else if (a16 && l == 1) RD_TRY(launch_conv_a16(h, h->plans[pl], h->d_plans + pl, B, in, d1_weights(h, dp), h->dch[l], dst, ep, st,
                             RDGAN_TAG_CRITIC_GEMM, false, true));
    else if (a16) RD_TRY(launch_conv16(h, h->plans[pl], h->d_plans + pl, B, in, h->bWF[l], dst, ep, st, RDGAN_TAG_CRITIC_GEMM, h->conv_f16 ? h->fWF[l] : nullptr));
    else RD_TRY(launch_conv(h, h->plans[pl], h->d_plans + pl, B, in, l == 1 ? d1_weights(h, dp) : dp + h->doff[2 * (l - 1)],
                         h->dch[l], dst, ep, st, RDGAN_TAG_CRITIC_GEMM));
    in = dst;
  }
  return 0;
}

// weight gradients over the 3B batch: inputs [h_real; h_fake; r_hat], output grads [u_real; u_fake; u_hat]
static int critic_weight_grads(rdgan_handle* h, float* grad, int B, hipStream_t st) {
  const bool a16 = h->a16 != 0;
  const int NBt = 3 * B;
  for (int l = 1; l <= 4; ++l) {
    int pl = l == 1 ? PL_D1F : PL_D2F + l - 2;
    const float* in = l == 1 ? h->cin : h->dh[l - 1];
    const bool padded = l == 1 && h->CP != h->Cin;   // D1 with padding channels: gradient of the padded kernel, then drop the pad rows
    const SlabRec rec = {pl, plan_flops(h->plans[pl], NBt), RDGAN_TAG_CRITIC_GEMM};
    if (l == 1 && d1_gemm_ok(h)) {
      RD_TRY(launch_d1_wgrad(h, in, h->du[1], grad + h->doff[0], NBt, st, grad + h->doff[1], (long)2 * B * h->dL[1]));
    } else if (l == 2 && d2_wgrad_slab_on(h)) {
      RD_TRY(launch_d2_wgrad_slab(h, rec, in, h->du[2], h->wpartial, h->wpartial_cap, grad + h->doff[2], NBt, nullptr, st));
    } else if (l == 2 && d2_wgrad_slab_t_on(h)) {
      const RdD2wGeom geo = {h->ddim[1][1], h->ddim[1][2], h->ddim[2][1], h->ddim[2][2], h->ddim[2][1] / 4, h->ddim[2][2] / 4};
      RD_TRY(launch_d2_wgrad_slab(h, rec, in, h->du[2], h->wpartial, h->wpartial_cap, grad + h->doff[2], NBt, &geo, st));
    } else if (l == 3 && d3_wgrad_slab_on(h)) {
      RD_TRY(launch_d3_wgrad_slab(h, rec, in, h->du[3], h->wpartial, h->wpartial_cap, grad + h->doff[4], NBt, st));
    } else if (a16 && l >= 2) {      // layers 2-4: bf16 activations against bf16 output gradients (on the border-class boxes)
      pl = critic_wgrad_plan(h, l, NBt);
      if (!wgrad16_ok(h->plans[pl], NBt)) return bad_arg(h, "bf16 storage mode: no bf16 weight-gradient tile for this critic layer");
      RD_TRY(launch_wgrad16(h, h->plans[pl], h->d_plans + pl, NBt, in, h->du[l], grad + h->doff[2 * (l - 1)], h->wpartial,
                            h->wpartial_cap, st, RDGAN_TAG_CRITIC_GEMM));
    } else {
      // fp32 storage, layers 2-4: the border-class boxes of the layer's forward plan (k_wgrad_gemm_ws<128,128> + k_wgrad_reduce_box)
      if (l >= 2 && !a16 && h->wave_spec) pl = critic_wgrad_plan(h, l, NBt);
      RD_TRY(launch_wgrad(h, h->plans[pl], h->d_plans + pl, NBt, in, h->du[l], padded ? h->dW1P : grad + h->doff[2 * (l - 1)],
                          h->wpartial, h->wpartial_cap, st, RDGAN_TAG_CRITIC_GEMM, a16));
    }
    if (padded) hipLaunchKernelGGL(k_unpad_w1, dim3(27), dim3(256), 0, st, h->dW1P, grad + h->doff[0], h->Cin, h->CP);
  }
  return 0;
}

// Dense weight gradient (row slices where the batch is large), then the losses
static int critic_dense_grad_and_losses(rdgan_handle* h, float* grad, int B, hipStream_t st) {
  const int NBt = 3 * B;
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_critic_dense_wgrad(h->a16 != 0, h->dh[4], grad + h->doff[8], h->dw6_part, NBt, h->F, B, dense_wgrad_slices(h->dense_slices, NBt), st);
    // (grad[doff[9]] = sum of dv over real|fake = 0, cleared by the loss kernel together with the unused loss slots)
    launch_critic_losses(h->v, h->gpv, grad + h->n_critic, B, h->d_flag, grad + h->doff[9], st);
  }
  RD_CHECK(h, hipGetLastError());
  return 0;
}

extern "C" int rdgan_critic_grad(rdgan_handle* h, const float* dp, const float* gp, const float* x_real,
                                 const float* cond, const float* z, uint64_t seed, float* grad, int B, void* stream) {
  return rdgan_critic_grad_after(h, dp, gp, x_real, cond, z, seed, grad, B, nullptr, stream);
}

extern "C" int rdgan_critic_grad_after(rdgan_handle* h, const float* dp, const float* gp, const float* x_real,
                                       const float* cond, const float* z, uint64_t seed, float* grad, int B,
                                       void* critic_ready_event, void* stream) {
  return rdgan_critic_grad_ahead(h, dp, gp, x_real, cond, z, seed, grad, B, critic_ready_event, nullptr, nullptr, 0, stream);
}

extern "C" int rdgan_critic_grad_ahead(rdgan_handle* h, const float* dp, const float* gp, const float* x_real,
                                       const float* cond, const float* z, uint64_t seed, float* grad, int B,
                                       void* critic_ready_event, const float* gen_z, const float* gen_cond, int gen_B,
                                       void* stream) {
  if (!h || !dp || !gp || !x_real || !cond || !z || !grad) return bad_arg(h, "critic_grad: null pointer");
  if (B < 1 || B > h->MB) return bad_arg(h, "critic_grad: B outside [1, max_batch]");
  if ((gen_z != nullptr) != (gen_cond != nullptr)) return bad_arg(h, "critic_grad: gen_z and gen_cond go together");
  if (gen_z && (gen_B < 1 || gen_B > h->MB)) return bad_arg(h, "critic_grad: gen_B outside [1, max_batch]");
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ahead_drain(h, st));
  const int NBt = 3 * B;
  // fake = G(z, cond), generator frozen (T:363,370): reads no critic weight, so it is issued in front of the wait for
  // them -- the previous critic update's all-reduce + Adam (on the caller's other stream) hide behind it
  // The weight-only kernels (generator weight forms, then the critic's transposes / bf16 images behind the "critic ready"
  // event) go to the side stream beside the generator forward; the compute stream waits for them where it needs them.
  hipStream_t ws = side_fork(h, st);
  RD_TRY(gen_forward_impl(h, gp, z, cond, h->fake, B, st, ws, false));    // nothing differentiates through the generator here
  if (critic_ready_event) RD_CHECK(h, hipStreamWaitEvent(ws, (hipEvent_t)critic_ready_event, 0));
  RD_TRY(prep_critic_weights(h, dp, ws));
  RD_TRY(side_join(h, st, h->ev_cw));
  // [real; fake; alpha*real + (1-alpha)*fake] with the condition as 2nd channel (T:275-282, T:376)
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_build_critic_input(h, x_real, h->fake, cond, B, 0, rd_make_key(seed, RD_STREAM_ALPHA), (uint32_t)h->sample_offset, st);
  }
  // the next generator step's forward, beside everything below (nothing below reads a generator buffer)
  if (gen_z && fwd_ahead_on(h)) RD_TRY(ahead_issue(h, gp, gen_z, gen_cond, gen_B, st));
  RD_TRY(critic_forward_impl(h, dp, NBt, seed, st));           // T:372,373,379 as one batch
  RD_TRY(critic_dgrad_chain(h, dp, NBt, B, 0, seed, st));       // dL/dh for real|fake, dD/dh for x_hat
  RD_TRY(critic_bias_grads(h, grad, B, st));                    // (side stream, joined below)
  // gradient penalty (T:238-241, T:382): g0 = dD/dx_hat, n = ||g0||, r0 = d(10 mean((n-1)^2))/dg0
  float* cin_hat = h->cin + (long)2 * B * h->dL[0] * h->CP;
  RD_TRY(critic_penalty_input(h, dp, act_off(h, h->du[1], (long)2 * B * h->dL[1] * 64), B, cin_hat, st));
  RD_TRY(critic_second_sweep(h, dp, cin_hat, B, seed, st));
  RD_TRY(critic_weight_grads(h, grad, B, st));
  RD_TRY(side_join(h, st, h->ev_join));                 // the bias-gradient sums issued on the side stream above
  return critic_dense_grad_and_losses(h, grad, B, st);
}

// ------------------------------------------------------------------------------------
// generator step gradients (T:395-408)
// ------------------------------------------------------------------------------------
// ---- stages of the backward through the generator (rdgan_gen_grad_after), from g0 = dL/d fake
// softmax backward, then the last conv (64 -> 1, T:345): weight grad [27][64], input grad (im2col route; the direct route's is
// part of block 3's PixelNorm backward, gen_block_pn_bwd), bias grad
static int gen_last_conv_bwd(rdgan_handle* h, const GenPass& s, const float* gp, float* grad, int B, hipStream_t st) {
  const int nd = h->nd;
  const long npix3 = (long)B * h->gpix[3];
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_softmax_bwd(h->fake, h->g0, h->dl, B, nd, nd, st);
  }
  if (s.a16 && !s.g9_direct) return bad_arg(h, "bf16 storage mode needs the direct backward of the last conv (g9_direct)");
  if (s.g9_direct) {
    RD_TRY(ensure_lds(h, s.a16 ? (const void*)k_g9_bwd_pairs<rd_bf16_t> : (const void*)k_g9_bwd_pairs<float>, 96 * 1024));
    // weight gradient on the matrix pipe, the h3 tensor streamed once (rdgan_edge.hip.h), where its partial rows fit
    const bool mfma = h->edge_kernels && g9w_mfma_ok(nd, npix3) && g9w_partial_floats(g9w_groups(true, B, nd)) <= h->wpartial_cap;
    RD_TRY(launch_g9_wgrad(h, {PL_G9B, 2.0 * npix3 * 64 * 27, RDGAN_TAG_GCONV_WGRAD}, mfma, s.a16, h->dl, h->h3, h->wpartial, h->wpartial_cap,
                           grad + h->goff[8], B, nd, st));
  } else {
    {
      ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
      hipLaunchKernelGGL(k_dl_im2col, dim3(ew_blocks(npix3 * 8)), dim3(256), 0, st, h->dl, h->P9, B, RDGAN_NHOURS, nd, nd);
    }
    RD_TRY(launch_wgrad(h, h->plans[PL_G9B], h->d_plans + PL_G9B, B, h->P9, h->h3, grad + h->goff[8], h->wpartial, h->wpartial_cap, st, RDGAN_TAG_GCONV_WGRAD));
    RD_TRY(launch_conv(h, h->plans[PL_G9B], h->d_plans + PL_G9B, B, h->P9, gp + h->goff[8], 64, h->gh3, epi_make(RD_EPI_PLAIN), st, RDGAN_TAG_GCONV_DGRAD));
  }
  // bias gradient of the last conv = sum of dl: on the side stream (dl is not written again in this call)
  hipStream_t cs = side_fork(h, st);
  RD_TRY(launch_colsum(h, h->dl, npix3 / 64, 64, h->g9b_tmp, cs));   // 64 partial sums of dl (npix3 % 64 == 0)
  RD_TRY(launch_colsum(h, h->g9b_tmp, 64, 1, grad + h->goff[9], cs));
  return 0;
}

// collapsed form: the input-gradient forms Wd[q][Cout][Cin] <- Wc (written by the forward unless that block ran in the shared-centre form)
static int gen_build_dgrad_forms(rdgan_handle* h, const GenPass& s, const float* gp, hipStream_t st) {
  if (!s.col) return 0;
  RdSliceMap map;
  collapsed_dgrad_slice_map(map.src);
  for (int l = 1; l <= 3; ++l) {
    if (gen_block_fast(h, l, fast_bwd_on(h))) continue;
    if (gen_block_fast(h, l, fast_fwd_on(h))) launch_collapse_weights(gp + h->goff[2 * l], h->GWC[l], (long)h->gch[l - 1] * h->gch[l], st);
    if (s.a16) continue;              // (bf16 storage: the input gradient reads the bf16 image of Wc re-ordered by tap: gen_block_bwd_collapsed)
    hipLaunchKernelGGL(k_transpose_map, dim3((h->gch[l] + 31) / 32, (h->gch[l - 1] + 31) / 32, 64), dim3(256), 0, st,
                       h->GWC[l], h->GWD[l], h->gch[l - 1], h->gch[l], map);
  }
  return 0;
}

// PixelNorm + LeakyReLU backward of block l: dys[l] from the gradient wrt the block output.  dE_in ("combine_dx_fused"): block
// l + 1 has left gups[l + 1] without its difference part, which this pass folds in
static int gen_block_pn_bwd(rdgan_handle* h, const GenPass& s, const float* gp, int l, int B, const float* dE_in, hipStream_t st) {
  const int nd = h->nd;
  const bool a16 = s.a16, fast = gen_block_fast(h, l, fast_bwd_on(h));
  ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
  if (l == 3 && s.g9_direct) {
    // input gradient of the 64 -> 1 conv + block 3's PixelNorm+LeakyReLU backward (+ plane-pair sums)
    if (g9_bwd_mfma_on(h)) {
      const int PP = nd <= 16 ? 4 : 1;        // plane pairs per unit (ten staged planes = 13 KB at ndomain 16; 3 B units deal evenly to 768 workgroups)
      const size_t lds9 = (size_t)(2 * PP + 2) * (nd + 2) * (nd + 2) * sizeof(float);
      const int nunits = B * (RDGAN_NHOURS / 2 / PP);
      RD_TRY(ensure_lds(h, (const void*)k_g9_bwd_mfma16, lds9));
      hipLaunchKernelGGL(k_g9_bwd_mfma16, dim3((unsigned)std::min(nunits, PP > 1 ? 768 : 1536)), dim3(256), lds9, st, h->dl, gp + h->goff[8],
                         (const rd_bf16_t*)s.hs[3], s.rs[3], (rd_bf16_t*)s.dys[3], nunits, RDGAN_NHOURS, nd, nd, PP);
    } else if (a16) hipLaunchKernelGGL(k_g9_bwd_pairs<rd_bf16_t>, dim3(B * (RDGAN_NHOURS / 2)), dim3(256), g9_pairs_lds(h), st, h->dl, gp + h->goff[8],
                         (const rd_bf16_t*)s.hs[3], s.rs[3], (rd_bf16_t*)s.dys[3], fast ? (rd_bf16_t*)h->fgS : (rd_bf16_t*)nullptr, RDGAN_NHOURS, nd, nd);
    else hipLaunchKernelGGL(k_g9_bwd_pairs<float>, dim3(B * (RDGAN_NHOURS / 2)), dim3(256), g9_pairs_lds(h), st, h->dl, gp + h->goff[8],
                         (const float*)s.hs[3], s.rs[3], s.dys[3], fast ? h->fgS : (float*)nullptr, RDGAN_NHOURS, nd, nd);
    RD_CHECK(h, hipGetLastError());
  } else if (fast) {     // ... and the sums of the output-gradient plane pairs the shared-centre form reads
    const long HW = (long)h->gdim[l][1] * h->gdim[l][2];
    RD_TRY(launch_pn_bwd_pairs(h, l == 3 ? h->gh3 : s.gups[l + 1], s.hs[l], s.rs[l], s.dys[l], h->fgS, (long)B * h->gdim[l - 1][0] * HW,
                               HW, h->gch[l], st, a16, l == 3 ? nullptr : dE_in, h->gdim[l - 1][0]));
  } else if (l == 3) RD_TRY(launch_pn_bwd(h, h->gh3, s.hs[3], s.rs[3], s.dys[3], (long)B * h->gpix[3], 64, 0, 0, 0, 0, st, a16));
  else RD_TRY(launch_pn_bwd(h, s.gups[l + 1], s.hs[l], s.rs[l], s.dys[l], (long)B * h->gpix[l], h->gch[l], s.col ? 0 : 1,
                         h->gdim[l][0], h->gdim[l][1], h->gdim[l][2], st, a16, dE_in));
  return 0;
}

// block l in the shared-centre form along d: E = d-differences of the block input, gS = sums of the output-gradient plane pairs.
// *dE_out: the gradient wrt E where the next PixelNorm backward is to fold it into dx (else it has been folded here)
static int gen_block_bwd_shared_centre(rdgan_handle* h, const GenPass& s, const float* gp, float* grad, int l, int B, const float** dE_out, hipStream_t st) {
  const bool a16 = s.a16;
  float* const* hs = s.hs;
  float* const* dys = s.dys;
  float* const* gups = s.gups;
  const long cc = (long)h->gch[l - 1] * h->gch[l];
  const int* sd = h->gdim[l - 1];
  const int D = sd[0];
  const long P = (long)sd[1] * sd[2] * h->gch[l - 1];
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    if (!gen_block_fast(h, l, fast_fwd_on(h))) {      // (otherwise the forward pass has left both)
      launch_diff_d(s, hs[l - 1], h->fE[l], B, D, P, st);
      launch_weight_transform(gp + h->goff[2 * l], h->fU[l], cc, st);
    }
  }
  // weight gradients of the three tap groups: E[s] x even planes, x x plane sums, E[s+1] x odd planes
  const float* wsrc[3] = {h->fE[l], hs[l - 1], h->fE[l]};
  const float* wdy[3] = {dys[l], h->fgS, dys[l]};
  for (int g = 0; g < 3; ++g) {
    int pl = PL_F1WA + 3 * g + l - 1;
    if (!a16 && gen_wgrad_boxes_on(h, pl, PL_F1WAX + 3 * g + l - 1)) pl = PL_F1WAX + 3 * g + l - 1;      // fp32 storage: the border boxes
    if (a16) {
      if (!wgrad16_ok(h->plans[pl], B)) return bad_arg(h, "bf16 storage mode: no bf16 weight-gradient tile for this block");
      RD_TRY(launch_wgrad16(h, h->plans[pl], h->d_plans + pl, B, wsrc[g], wdy[g], h->fdU, h->wpartial, h->wpartial_cap, st, RDGAN_TAG_GCONV_WGRAD));
    } else RD_TRY(launch_wgrad(h, h->plans[pl], h->d_plans + pl, B, wsrc[g], wdy[g], h->fdU, h->wpartial, h->wpartial_cap, st, RDGAN_TAG_GCONV_WGRAD));
  }
  launch_weight_transform_adj(h->fdU, grad + h->goff[2 * l], cc, st);
  RD_TRY(launch_colsum(h, dys[l], (long)B * h->gpix[l], h->gch[l], grad + h->goff[2 * l + 1], side_fork(h, st), a16));   // bias gradient, beside the GEMMs (dys[l] is read-only from here on)
  // input gradients: the shared part from gS, the difference part dE from dy
  const int pbs = PL_F1BS + l - 1, pbe = PL_F1BE + l - 1;
  RdEpi eb = epi_make(RD_EPI_PLAIN);
  eb.out16 = a16;
  RdSliceMap map;
  fastd_dgrad_slice_map(map.src);
  if (a16) {
    // the forward forms U re-ordered by tap ([Cin][Cout] is already the [N][K] layout of these GEMMs)
    {
      ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
      hipLaunchKernelGGL(k_blocks_to_bf16, dim3((unsigned)std::min<long>((cc / 8 + 255) / 256, 64), 48), dim3(256), 0, st,
                         h->fU[l], (unsigned short*)h->bUT, cc, map);
    }
    RD_TRY(launch_conv16(h, h->plans[pbs], h->d_plans + pbs, B, h->fgS, h->bUT, gups[l], eb, st, RDGAN_TAG_GCONV_DGRAD));
    RD_TRY(launch_conv16(h, h->plans[pbe], h->d_plans + pbe, B, dys[l], h->bUT, h->fdE, eb, st, RDGAN_TAG_GCONV_DGRAD));
  } else {
    hipLaunchKernelGGL(k_transpose_map, dim3((h->gch[l] + 31) / 32, (h->gch[l - 1] + 31) / 32, 48), dim3(256), 0, st, h->fU[l],
                       h->fUT, h->gch[l - 1], h->gch[l], map);
    RD_TRY(launch_conv(h, h->plans[pbs], h->d_plans + pbs, B, h->fgS, h->fUT, h->gch[l - 1], gups[l], eb, st, RDGAN_TAG_GCONV_DGRAD));
    RD_TRY(launch_conv(h, h->plans[pbe], h->d_plans + pbe, B, dys[l], h->fUT, h->gch[l - 1], h->fdE, eb, st, RDGAN_TAG_GCONV_DGRAD));
  }
  // dx += adjoint of the differencing of dE: by the PixelNorm backward of block l - 1 (fp32 storage: both of its kernels take
  // dE; nothing else reads the combined dx), else in a pass of its own
  if (!a16 && h->combine_dx_fused && l >= 2) *dE_out = h->fdE;
  else {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_combine_dx(a16, gups[l], h->fdE, B, D, P, st);
  }
  return 0;
}

// block l in the collapsed form (8 taps per phase on the source grid): weight gradient folded back to 27 taps, bias, input gradient
static int gen_block_bwd_collapsed(rdgan_handle* h, const GenPass& s, float* grad, int l, int B, hipStream_t st) {
  const bool a16 = s.a16;
  const float* x = s.hs[l - 1];
  const float* dy = s.dys[l];
  const long cc = (long)h->gch[l - 1] * h->gch[l];
  int plf = PL_G1FC + l - 1, plb = gen_box_plan(h, PL_G1BC + l - 1, PL_G1BCX + l - 1, B);
  const int plfx = PL_G1FCX + l - 1;
  const bool wbox = gen_wgrad_boxes_on(h, plf, plfx);      // weight gradient through the streaming kernels: as the shared-centre ones
  bool bias_done = false;         // (the slab kernels deliver the bias gradient too)
  if (upwgrad_slab_on(h, l)) {
    const SlabRec rec = {plf, plan_flops(h->plans[plf], B), RDGAN_TAG_GCONV_WGRAD};
    if (l == 3)     // each workgroup owns one phase and keeps its eight tap products in registers over its share of the batch
      RD_TRY(launch_upconv_wgrad_slab(h, rec, x, dy, h->wpartial, h->wpartial_cap, h->dWc, h->ubias_part, grad + h->goff[2 * l + 1], B, st));
    else            // the same on block 2's geometry: a workgroup owns (phase, quarter of the 256 input channels)
      RD_TRY(launch_upconv2_wgrad_slab(h, rec, x, dy, h->wpartial, h->wpartial_cap, h->dWc, h->ubias_part, grad + h->goff[2 * l + 1], B, st));
    bias_done = true;
  } else if (a16) {
    if (wbox && wgrad16_ok(h->plans[plfx], B)) plf = plfx;
    if (!wgrad16_ok(h->plans[plf], B)) return bad_arg(h, "bf16 storage mode: no bf16 weight-gradient tile for this block");
    RD_TRY(launch_wgrad16(h, h->plans[plf], h->d_plans + plf, B, x, dy, h->dWc, h->wpartial, h->wpartial_cap, st, RDGAN_TAG_GCONV_WGRAD));
  } else {
    if (wbox) plf = plfx;
    RD_TRY(launch_wgrad(h, h->plans[plf], h->d_plans + plf, B, x, dy, h->dWc, h->wpartial, h->wpartial_cap, st, RDGAN_TAG_GCONV_WGRAD));
  }
  launch_fold_collapsed_wgrad(h->dWc, grad + h->goff[2 * l], cc, st);
  if (!bias_done)
    RD_TRY(launch_colsum(h, dy, (long)B * h->gpix[l], h->gch[l], grad + h->goff[2 * l + 1], side_fork(h, st), a16));   // bias gradient, beside the GEMMs (dys[l] is read-only from here on)
  if (a16) {      // the collapsed forms re-ordered by tap are already [N = Cin][K = Cout]
    RdSliceMap map;
    collapsed_dgrad_slice_map(map.src);
    hipLaunchKernelGGL(k_blocks_to_bf16, dim3((unsigned)std::min<long>((cc / 8 + 255) / 256, 64), 64), dim3(256), 0, st,
                       h->GWC[l], (unsigned short*)h->bG1B, cc, map, h->conv_f16 ? (unsigned short*)h->fG1B : nullptr, h->gch[l]);
    RdEpi eb = epi_make(RD_EPI_PLAIN);
    eb.out16 = 1;
    RD_TRY(launch_conv16(h, h->plans[plb], h->d_plans + plb, B, dy, h->bG1B, s.gups[l], eb, st, RDGAN_TAG_GCONV_DGRAD, h->conv_f16 ? h->fG1B : nullptr));
  } else RD_TRY(launch_conv(h, h->plans[plb], h->d_plans + plb, B, dy, h->GWD[l], h->gch[l - 1], s.gups[l], epi_make(RD_EPI_PLAIN), st, RDGAN_TAG_GCONV_DGRAD));
  return 0;
}

// block l in the direct 27-tap form ("collapse" off): the gradient wrt the block input stays on the upsampled grid
static int gen_block_bwd_direct(rdgan_handle* h, const GenPass& s, float* grad, int l, int B, hipStream_t st) {
  const int plf = PL_G1F + l - 1, plb = PL_G1B + l - 1;
  RD_TRY(launch_wgrad(h, h->plans[plf], h->d_plans + plf, B, s.hs[l - 1], s.dys[l], grad + h->goff[2 * l], h->wpartial, h->wpartial_cap, st, RDGAN_TAG_GCONV_WGRAD));
  RD_TRY(launch_colsum(h, s.dys[l], (long)B * h->gpix[l], h->gch[l], grad + h->goff[2 * l + 1], side_fork(h, st)));
  RD_TRY(launch_conv(h, h->plans[plb], h->d_plans + plb, B, s.dys[l], h->GWT[l], h->gch[l - 1], s.gups[l], epi_make(RD_EPI_PLAIN), st, RDGAN_TAG_GCONV_DGRAD));
  return 0;
}

// Dense (T:326): (pool the upsample adjoint,) LeakyReLU', then dW = xcat^T ga0, db = colsum(ga0)
static int gen_dense_bwd(rdgan_handle* h, const GenPass& s, float* grad, int B, hipStream_t st) {
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    if (s.col) launch_lrelu_bwd(s.a16, h->gup1, h->h0, h->ga0, (long)B * h->gpix[0] * 64, st);
    else launch_pool_lrelu_bwd(h->gup1, h->h0, h->ga0, B, h->gdim[0][0], h->gdim[0][1], h->gdim[0][2], 256, st);
  }
  RD_TRY(launch_wgrad(h, h->plans[PL_GDENSE], h->d_plans + PL_GDENSE, B, h->xcat, h->ga0, grad + h->goff[0], h->wpartial,
                      h->wpartial_cap, st, RDGAN_TAG_GCONV_WGRAD));
  return launch_colsum(h, h->ga0, B, h->n_nodes, grad + h->goff[1], side_fork(h, st));   // (same stream as the other column sums: they share their scratch)
}

extern "C" int rdgan_gen_grad(rdgan_handle* h, const float* dp, const float* gp, const float* z, const float* cond,
                              uint64_t seed, float* grad, int B, void* stream) {
  return rdgan_gen_grad_after(h, dp, gp, z, cond, seed, grad, B, nullptr, stream);
}

extern "C" int rdgan_gen_grad_after(rdgan_handle* h, const float* dp, const float* gp, const float* z, const float* cond,
                                    uint64_t seed, float* grad, int B, void* critic_ready_event, void* stream) {
  if (!h || !dp || !gp || !z || !cond || !grad) return bad_arg(h, "gen_grad: null pointer");
  if (B < 1 || B > h->MB) return bad_arg(h, "gen_grad: B outside [1, max_batch]");
  hipStream_t st = (hipStream_t)stream;
  // the forward issued by the last critic step (rdgan_critic_grad_ahead) is this step's when it was made from the same
  // generator slab (pointer and content version), latent and condition buffers and batch size; otherwise it is dropped
  const bool ahead = h->ahead_pending && gp == h->ahead_gp && z == h->ahead_z && cond == h->ahead_cond && B == h->ahead_B &&
                     h->gver_in == h->ahead_gver;
  if (!ahead) RD_TRY(ahead_drain(h, st));
  h->ahead_pending = false;
  h->gate_keep_B = 0;
  if (!h->collapse)
    for (int l = 1; l <= 3; ++l)
      RD_TRY(launch_transpose(h, gp + h->goff[2 * l], h->GWT[l], 27, h->gch[l - 1], h->gch[l], h->gch[l - 1], st));
  // the generator forward reads no critic weight: the last critic update (all-reduce + Adam on the caller's other
  // stream) hides behind it; everything below the wait reads them
  hipStream_t ws = side_fork(h, st);                    // weight-only kernels beside the generator forward (see rdgan_critic_grad_after)
  if (!ahead) RD_TRY(gen_forward_impl(h, gp, z, cond, h->fake, B, st, ws));
  if (critic_ready_event) RD_CHECK(h, hipStreamWaitEvent(ws, (hipEvent_t)critic_ready_event, 0));
  RD_TRY(prep_critic_weights(h, dp, ws));
  RD_TRY(side_join(h, st, h->ev_cw));
  if (ahead) {      // the early forward's outputs, and its non-finite flag as this call's
    RD_CHECK(h, hipStreamWaitEvent(st, h->ev_ahead_done, 0));
    std::swap(h->d_flag, h->flag_ahead);
  }
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_build_critic_input(h, nullptr, h->fake, cond, B, 1, 0u, 0u, st);
  }
  RD_TRY(critic_forward_impl(h, dp, B, seed, st));              // critic frozen, dropout active (T:395,405)
  RD_TRY(critic_dgrad_chain(h, dp, B, B, 1, seed, st));
  RD_TRY(critic_input_grad(h, dp, h->du[1], B, st));                 // g0 = dL/d fake
  // back through the generator: the last conv, then three [upsample, conv, pixelnorm, lrelu] blocks, last to first, then Dense
  const GenPass s = gen_pass(h, B);
  RD_TRY(gen_last_conv_bwd(h, s, gp, grad, B, st));
  RD_TRY(gen_build_dgrad_forms(h, s, gp, st));
  const float* dE = nullptr;      // block l + 1's gradient wrt its hour differences, handed to block l's PixelNorm backward
  for (int l = 3; l >= 1; --l) {
    RD_TRY(gen_block_pn_bwd(h, s, gp, l, B, dE, st));
    dE = nullptr;
    // shared-centre backward only where the hour axis is long enough to pay for its (D+1)/D boundary plane
    if (gen_block_fast(h, l, fast_bwd_on(h))) RD_TRY(gen_block_bwd_shared_centre(h, s, gp, grad, l, B, &dE, st));
    else if (s.col) RD_TRY(gen_block_bwd_collapsed(h, s, grad, l, B, st));
    else RD_TRY(gen_block_bwd_direct(h, s, grad, l, B, st));
  }
  RD_TRY(gen_dense_bwd(h, s, grad, B, st));
  RD_TRY(side_join(h, st, h->ev_join));                // the bias-gradient sums issued on the side stream above
  {
    ProfScope ps(h, RDGAN_TAG_ELEMENTWISE, st);
    launch_gen_loss(h->v, grad + h->n_gen, B, h->d_flag, st);
  }
  RD_CHECK(h, hipGetLastError());
  return 0;
}

extern "C" int rdgan_adam(float* params, const float* grad, float* v, long n, int t, float lr, float beta2, float eps,
                          float grad_scale, void* stream) {
  if (!params || !grad || !v || n < 1 || t < 1) return -2;
  float lr_t = lr * sqrtf(1.0f - powf(beta2, (float)t));
  hipLaunchKernelGGL(k_adam, dim3(ew_blocks(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, params, grad, v, n, lr_t, beta2,
                     eps, grad_scale);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// op-level entry points for the parity tests
// ------------------------------------------------------------------------------------
struct TmpPlan {
  RdPlan host; RdPlan* dev = nullptr; RdRow* tab = nullptr;
  int upload() {
    std::vector<RdRow> t;
    if (!plan_build_tables(host, t)) return -2;
    hipError_t e = hipMalloc((void**)&tab, sizeof(RdRow) * t.size());
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(tab, t.data(), sizeof(RdRow) * t.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int)e;
    host.tab = tab;
    e = hipMalloc((void**)&dev, sizeof(RdPlan));
    if (e != hipSuccess) return (int)e;
    return (int)hipMemcpy(dev, &host, sizeof(RdPlan), hipMemcpyHostToDevice);
  }
  ~TmpPlan() { if (dev) (void)hipFree(dev); if (tab) (void)hipFree(tab); }
};

// The device buffers of one op-level call: freed when the call returns.  `rc` keeps the first failing HIP call; once it is set
// the later requests do nothing and return nullptr, so an entry allocates all it needs and checks `rc` once.
struct TmpBufs {
  std::vector<void*> bufs; int rc = 0;
  void* bytes(size_t n) {
    void* p = nullptr;
    if (rc == 0 && (rc = (int)hipMalloc(&p, n)) == 0) bufs.push_back(p);
    return rc == 0 ? p : nullptr;
  }
  float* floats(size_t n) { return (float*)bytes(n * sizeof(float)); }
  void* bf16(long n) { return bytes((size_t)n * 2); }
  // a fresh bf16 buffer holding the fp32 array `in`, rounded to nearest even
  void* to_bf16(const float* in, long n, hipStream_t st) {
    void* p = bf16(n);
    if (rc == 0) rc = launch_to_bf16(nullptr, in, p, n, st);
    return p;
  }
  ~TmpBufs() { for (void* p : bufs) (void)hipFree(p); }
};
// widen a bf16 buffer into the caller's fp32 output
static int launch_widen_bf16(const void* in, float* out, long n, hipStream_t st) {
  hipLaunchKernelGGL(k_bf16_to_f32, dim3(ew_blocks(n)), dim3(256), 0, st, (const rd_bf16_t*)in, out, n);
  return (int)hipGetLastError();
}

extern "C" int rdgan_op_conv3d(const float* x, const float* w, const float* bias, float* y, int B, int D, int H, int W,
                               int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h, int pad_w,
                               int upsample, void* stream) {
  if (!x || !w || !y || Cin % 4 || (Cout % 64 && Cout != 32)) return -2;
  TmpPlan tp;
  tp.host = plan_conv_fwd(D, H, W, Cin, Cout, Do, Ho, Wo, stride, pad_d, pad_h, pad_w, upsample);
  RD_TRY(tp.upload());
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(launch_conv(nullptr, tp.host, tp.dev, B, x, w, Cout, y, epi_make(bias ? RD_EPI_BIAS : RD_EPI_PLAIN, bias), st, -1));
  return (int)hipStreamSynchronize(st);
}

// weight gradient with bf16 operands (tests): x and gy rounded to bf16 on the device, fp32 accumulation.  Cin % 128 == 0,
// Cout % 64 == 0, no folded upsample.
extern "C" int rdgan_op_conv3d_wgrad_bf16(const float* x, const float* gy, float* dw, int B, int D, int H, int W, int Cin,
                                          int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h, int pad_w,
                                          void* stream) {
  if (!x || !gy || !dw || Cin % 64 || Cout % 64) return -2;
  hipStream_t st = (hipStream_t)stream;
  TmpPlan tp;
  tp.host = plan_conv_fwd(D, H, W, Cin, Cout, Do, Ho, Wo, stride, pad_d, pad_h, pad_w, 0);
  RD_TRY(tp.upload());
  if (!wgrad16_ok(tp.host, B)) return -2;
  const size_t need = std::max(wgrad_partial_need(tp.host, B), wgrad_partial_need(tp.host, B, true));
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * D * H * W * Cin, st);
  void* gb = t.to_bf16(gy, (long)B * Do * Ho * Wo * Cout, st);
  float* partial = t.floats(need);
  RD_TRY(t.rc);
  RD_TRY(launch_wgrad16(nullptr, tp.host, tp.dev, B, xb, gb, dw, partial, need, st, -1));
  return (int)hipStreamSynchronize(st);
}

// bf16-operand variant of the above for stride-1/2 convs without folded upsample (tests): x and w are rounded to
// bf16 (nearest even) on the device, products accumulate in fp32.  Cin % 64 == 0, Cout % 64 == 0.
extern "C" int rdgan_op_conv3d_bf16(const float* x, const float* w, const float* bias, float* y, int B, int D, int H, int W,
                                    int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h, int pad_w,
                                    int out_bf16, void* stream) {
  if (!x || !w || !y || Cin % 64 || Cout % 64) return -2;
  hipStream_t st = (hipStream_t)stream;
  TmpPlan tp;
  tp.host = plan_conv_fwd(D, H, W, Cin, Cout, Do, Ho, Wo, stride, pad_d, pad_h, pad_w, 0);
  RD_TRY(tp.upload());
  const long nw = 27L * Cin * Cout;
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * D * H * W * Cin, st);
  void* wb = t.bf16(nw);
  RD_TRY(t.rc);
  RD_TRY(launch_weights_to_bf16_t(nullptr, w, wb, 27, Cin, Cout, st));
  RdEpi ep = epi_make(bias ? RD_EPI_BIAS : RD_EPI_PLAIN, bias);
  ep.out16 = out_bf16 ? 1 : 0;
  void* wf = nullptr;
  if (out_bf16 == 2) {       // the fragment kernel (k_conv_gemm_f16), which must accept the launch
    if (!conv_f16_ok(nullptr, tp.host, B, ep)) return -2;
    wf = t.bf16(nw);
    RD_TRY(t.rc);
    RD_TRY(launch_wfrag_image(nullptr, wb, wf, 27, Cout, Cin, st));
  }
  RD_TRY(launch_conv16(nullptr, tp.host, tp.dev, B, xb, wb, y, ep, st, -1, wf));
  return (int)hipStreamSynchronize(st);
}

extern "C" int rdgan_op_conv3d_dgrad(const float* gy, const float* w, float* gx, int B, int D, int H, int W, int Cin,
                                     int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h, int pad_w,
                                     void* stream) {
  if (!gy || !w || !gx || Cout % 4 || Cin % 64) return -2;
  hipStream_t st = (hipStream_t)stream;
  TmpBufs t;
  float* wt = t.floats((size_t)27 * Cin * Cout);
  RD_TRY(t.rc);
  const int rc = launch_transpose(nullptr, w, wt, 27, Cin, Cout, Cin, st);
  TmpPlan tp;
  if (stride == 1) {
    if (pad_d != 1 || pad_h != 1 || pad_w != 1 || Do != D || Ho != H || Wo != W) return -2;
    tp.host = plan_conv_dgrad_s1(D, H, W, Cin, Cout);
  } else {
    int pad[3] = {pad_d, pad_h, pad_w};
    tp.host = plan_conv_dgrad_s2(D, H, W, Cin, Do, Ho, Wo, Cout, pad);
  }
  RD_TRY(rc);
  RD_TRY(tp.upload());
  RD_TRY(launch_conv(nullptr, tp.host, tp.dev, B, gy, wt, Cin, gx, epi_make(RD_EPI_PLAIN), st, -1));
  return (int)hipStreamSynchronize(st);
}

// input gradient with bf16 operands (tests): gy and w rounded to bf16, fp32 accumulation.  The [tap][Cin][Cout] kernel IS
// the [tap block][N][K] layout of this GEMM (N = Cin, K = Cout), so the weights are only converted.
extern "C" int rdgan_op_conv3d_dgrad_bf16(const float* gy, const float* w, float* gx, int B, int D, int H, int W, int Cin,
                                          int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h, int pad_w,
                                          void* stream) {
  if (!gy || !w || !gx || Cout % 64 || Cin % 64) return -2;
  hipStream_t st = (hipStream_t)stream;
  TmpPlan tp;
  if (stride == 1) {
    if (pad_d != 1 || pad_h != 1 || pad_w != 1 || Do != D || Ho != H || Wo != W) return -2;
    tp.host = plan_conv_dgrad_s1(D, H, W, Cin, Cout);
  } else {
    int pad[3] = {pad_d, pad_h, pad_w};
    tp.host = plan_conv_dgrad_s2(D, H, W, Cin, Do, Ho, Wo, Cout, pad);
  }
  TmpBufs t;
  void* gb = t.bf16((long)B * Do * Ho * Wo * Cout);
  void* wb = t.bf16(27L * Cin * Cout);
  RD_TRY(t.rc);
  RD_TRY(tp.upload());
  RD_TRY(launch_to_bf16(nullptr, gy, gb, (long)B * Do * Ho * Wo * Cout, st));
  RD_TRY(launch_to_bf16(nullptr, w, wb, 27L * Cin * Cout, st));
  RD_TRY(launch_conv16(nullptr, tp.host, tp.dev, B, gb, wb, gx, epi_make(RD_EPI_PLAIN), st, -1));
  return (int)hipStreamSynchronize(st);
}

extern "C" int rdgan_op_conv3d_wgrad(const float* x, const float* gy, float* dw, int B, int D, int H, int W, int Cin,
                                     int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h, int pad_w,
                                     int upsample, void* stream) {
  if (!x || !gy || !dw || Cin % 4 || Cout % 64) return -2;
  hipStream_t st = (hipStream_t)stream;
  TmpPlan tp;
  tp.host = plan_conv_fwd(D, H, W, Cin, Cout, Do, Ho, Wo, stride, pad_d, pad_h, pad_w, upsample);
  RD_TRY(tp.upload());
  const size_t need = wgrad_partial_need(tp.host, B);
  TmpBufs t;
  float* partial = t.floats(need);
  RD_TRY(t.rc);
  RD_TRY(launch_wgrad(nullptr, tp.host, tp.dev, B, x, gy, dw, partial, need, st, -1));
  return (int)hipStreamSynchronize(st);
}

// Weight gradient of one tap group of the shared-centre form through the production plan
// (plan_fastd_wgrad: 4 output-parity phases x 4 taps, an EVEN tap count, which is what lets the launcher pick the 256-row
// tile at B * D*H*W >= 65536): group g = 0: src = E [B,D+1,H,W,Cin] against the even planes of dy [B,2D,2H,2W,Cout];
// g = 1: src = x [B,D,H,W,Cin] against the plane-pair sums gS [B,D,2H,2W,Cout]; g = 2: E at j = s+1 against the odd planes.
// dU [48][Cin][Cout]: the 16 forms g*16 .. g*16+15 are written.  bf16 = 1: operands rounded to bf16 on the device
// (k_wgrad_gemm_ws16), fp32 accumulation and output.
extern "C" int rdgan_op_fastd_wgrad(const float* src, const float* dy, float* dU, int B, int D, int H, int W, int Cin, int Cout,
                                    int g, int bf16, void* stream) {
  if (!src || !dy || !dU || g < 0 || g > 2 || Cin % 4 || Cout % 64) return -2;
  hipStream_t st = (hipStream_t)stream;
  TmpPlan tp;
  tp.host = plan_fastd_wgrad(D, H, W, Cin, Cout, g);
  RD_TRY(tp.upload());
  const size_t need = std::max(wgrad_partial_need(tp.host, B), wgrad_partial_need(tp.host, B, true));
  TmpBufs t;
  float* partial = t.floats(need);
  RD_TRY(t.rc);
  if (bf16) {
    if (!wgrad16_ok(tp.host, B)) return -2;
    void* xb = t.to_bf16(src, (long)B * tp.host.src_sample, st);
    void* gb = t.to_bf16(dy, (long)B * tp.host.dst_sample, st);
    RD_TRY(t.rc);
    RD_TRY(launch_wgrad16(nullptr, tp.host, tp.dev, B, xb, gb, dU, partial, need, st, -1));
  } else {
    rdgan_handle fake_h;                   // (wave_spec = 1: the producer/consumer kernel, as in production)
    RD_TRY(launch_wgrad(&fake_h, tp.host, tp.dev, B, src, dy, dU, partial, need, st, -1));
  }
  return (int)hipStreamSynchronize(st);
}

// Weight gradient of the last generator conv (64 -> 1) alone, through the production kernels: kernel = 1 the matrix-pipe kernel
// (k_g9_wgrad_mfma), 0 the scalar kernel (k_g9_wgrad_pairs); bf16 = 1 rounds h3 to bf16 first (storage mode)
extern "C" int rdgan_op_g9_wgrad(const float* dl, const float* h3, float* dW, int B, int nd, int bf16, int kernel, void* stream) {
  if (!dl || !h3 || !dW || B < 1 || nd < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long npix = (long)B * RDGAN_NHOURS * nd * nd;
  if (npix >= 0x7FFFFFFFL) return -2;
  if (kernel && !g9w_mfma_ok(nd, npix)) return -2;
  const size_t need = g9w_partial_floats(g9w_groups(kernel != 0, B, nd));
  TmpBufs t;
  float* partial = t.floats(need);
  const void* hb = bf16 ? t.to_bf16(h3, npix * 64, st) : h3;
  RD_TRY(t.rc);
  RD_TRY(launch_g9_wgrad(nullptr, kOpRec, kernel != 0, bf16 != 0, dl, hb, partial, need, dW, B, nd, st));
  return (int)hipStreamSynchronize(st);
}

// Generator block 3 forward of the bf16 storage mode through the slab kernel alone (rdgan_upconv16.hip.h): x [B,12,8,8,128] and the
// Conv3D kernel w [3,3,3,128,64] are rounded to bf16 on the device (the kernel after the upsample collapse), y [B,24,16,16,64] =
// LeakyReLU(PixelNorm(upconv(x) + bias)) comes back as fp32 (the kernel's bf16 output widened), rinv [B,24,16,16]; dbg (optional,
// [B*24*16*16][4]): the row sums of squares and 1/l2 as both lane halves computed them.
extern "C" int rdgan_op_upconv_slab16(const float* x, const float* w, const float* bias, float* y, float* rinv, float* dbg, int B,
                                      void* stream) {
  if (!x || !w || !bias || !y || !rinv || B < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long ny = (long)B * 24 * 256 * 64;
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 12 * 64 * 128, st);
  void* yb = t.bf16(ny);
  void* wi = t.bytes(64L * 8 * 2 * 64 * 16);
  float* wc = t.floats(64L * 128 * 64);
  RD_TRY(t.rc);
  hipLaunchKernelGGL(k_collapse_weights, dim3(ew_blocks(16L * 128 * 64)), dim3(256), 0, st, w, wc, 128 * 64);
  launch_upconv_wimg(wc, wi, st);
  RD_TRY(launch_upconv_slab<0>(nullptr, kOpRec, xb, wi, bias, yb, rinv, B, dbg, nullptr, nullptr, true, st));
  RD_TRY(launch_widen_bf16(yb, y, ny, st));
  return (int)hipStreamSynchronize(st);
}

// The same block on source planes of H x W positions (multiples of 8) through the TILED slab kernel alone (rdgan_upconv16t.hip.h):
// x [B,12,H,W,128] -> y [B,24,2H,2W,64], rinv [B,24,2H,2W]; dbg (optional, [B*24*2H*2W][4]) as above.
extern "C" int rdgan_op_upconv_slab_t16(const float* x, const float* w, const float* bias, float* y, float* rinv, float* dbg, int B,
                                        int H, int W, void* stream) {
  if (!x || !w || !bias || !y || !rinv || B < 1 || H < 8 || W < 8 || (H & 7) || (W & 7)) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long ny = (long)B * 24 * 4 * H * W * 64;
  if (12L * H * W * 256 >= 0x7FFFFFF0L) return -2;
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 12 * H * W * 128, st);
  void* yb = t.bf16(ny);
  void* wi = t.bytes(64L * 8 * 2 * 64 * 16);
  float* wc = t.floats(64L * 128 * 64);
  RD_TRY(t.rc);
  hipLaunchKernelGGL(k_collapse_weights, dim3(ew_blocks(16L * 128 * 64)), dim3(256), 0, st, w, wc, 128 * 64);
  launch_upconv_wimg_t(wc, wi, st);
  RD_TRY(launch_upconv_slab_t(nullptr, kOpRec, xb, wi, bias, yb, rinv, B, H, W, dbg, nullptr, nullptr, true, st));
  RD_TRY(launch_widen_bf16(yb, y, ny, st));
  return (int)hipStreamSynchronize(st);
}

// Collapsed weight gradient of generator block 3 through the slab kernel alone (rdgan_upwgrad16.hip.h), ndomain 16: x [B,12,8,8,128]
// and dy [B,24,16,16,64] are rounded to bf16 on the device; dWc [64 = phase*8 + tap][128][64] fp32.
extern "C" int rdgan_op_upconv_wgrad_slab16(const float* x, const float* dy, float* dWc, int B, void* stream) {
  if (!x || !dy || !dWc || B < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const size_t need = upwgrad_partial_floats(upwgrad_groups(B));
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 12 * 64 * 128, st);
  void* yb = t.to_bf16(dy, (long)B * 24 * 256 * 64, st);
  float* part = t.floats(need);
  RD_TRY(t.rc);
  RD_TRY(launch_upconv_wgrad_slab(nullptr, kOpRec, xb, yb, part, need, dWc, nullptr, nullptr, B, st));
  return (int)hipStreamSynchronize(st);
}

// Forward of the critic's second layer through the slab kernel alone (rdgan_d2fwd16.hip.h), ndomain 16: x [B,11,7,7,64] and the layer's
// kernel w [3,3,3,64,128] are rounded to bf16 on the device; y [B,6,4,4,128] = dropout(LeakyReLU(conv(x; stride 2, 'same') + bias))
// comes back as fp32 (the bf16 output widened); seed = 0: no dropout, otherwise the layer-2 mask of `seed` (counter = flat index of y).
extern "C" int rdgan_op_d2_fwd_slab16(const float* x, const float* w, const float* bias, float* y, int B, uint64_t seed, void* stream) {
  if (!x || !w || !bias || !y || B < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long ny = (long)B * 96 * 128;
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 539 * 64, st);
  void* yb = t.bf16(ny);
  void* wi = t.bytes((size_t)RD_D2F_KSTEPS * 4 * 64 * 16);
  RD_TRY(t.rc);
  launch_d2f_wimg(w, wi, st);
  RD_TRY(launch_d2_fwd_slab(nullptr, kOpRec, xb, wi, bias, yb, B, seed != 0, rd_make_key(seed, RD_STREAM_D1 + 1), st));
  RD_TRY(launch_widen_bf16(yb, y, ny, st));
  return (int)hipStreamSynchronize(st);
}

// Weight gradient of the critic's third layer through the slab kernel alone (rdgan_d3wgrad16.hip.h), ndomain 16: x [B,6,4,4,128]
// (layer 2's output) and dy [B,3,2,2,256] are rounded to bf16 on the device; dW [3,3,3,128,256] fp32.
extern "C" int rdgan_op_d3_wgrad_slab16(const float* x, const float* dy, float* dW, int B, void* stream) {
  if (!x || !dy || !dW || B < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const size_t need = d3w_partial_floats(d3w_groups(B));
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 96 * 128, st);
  void* yb = t.to_bf16(dy, (long)B * 12 * 256, st);
  float* part = t.floats(need);
  RD_TRY(t.rc);
  RD_TRY(launch_d3_wgrad_slab(nullptr, kOpRec, xb, yb, part, need, dW, B, st));
  return (int)hipStreamSynchronize(st);
}

// Weight gradient of the critic's second layer through the slab kernel alone (rdgan_d2wgrad16.hip.h), ndomain 16: x [B,11,7,7,64]
// (layer 1's output) and dy [B,6,4,4,128] are rounded to bf16 on the device; dW [3,3,3,64,128] fp32.
extern "C" int rdgan_op_d2_wgrad_slab16(const float* x, const float* dy, float* dW, int B, void* stream) {
  if (!x || !dy || !dW || B < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const size_t need = d2w_partial_floats(d2w_groups(B));
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 539 * 64, st);
  void* yb = t.to_bf16(dy, (long)B * 96 * 128, st);
  float* part = t.floats(need);
  RD_TRY(t.rc);
  RD_TRY(launch_d2_wgrad_slab(nullptr, kOpRec, xb, yb, part, need, dW, B, nullptr, st));
  return (int)hipStreamSynchronize(st);
}

// The same through the tiled kernel (k_d2_wgrad_slab_t16): x [B,11,2 OH - 1,2 OW - 1,64], dy [B,6,OH,OW,128], OH and OW multiples of 4.
extern "C" int rdgan_op_d2_wgrad_slab_t16(const float* x, const float* dy, float* dW, int B, int OH, int OW, void* stream) {
  if (!x || !dy || !dW || B < 1 || OH < 4 || OW < 4 || OH % 4 || OW % 4) return -2;
  hipStream_t st = (hipStream_t)stream;
  const RdD2wGeom geo = {2 * OH - 1, 2 * OW - 1, OH, OW, OH / 4, OW / 4};
  const size_t need = d2w_partial_floats(d2w_groups((long)B * geo.TH * geo.TW));
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 11 * geo.IH * geo.IW * 64, st);
  void* yb = t.to_bf16(dy, (long)B * 6 * OH * OW * 128, st);
  float* part = t.floats(need);
  RD_TRY(t.rc);
  RD_TRY(launch_d2_wgrad_slab(nullptr, kOpRec, xb, yb, part, need, dW, B, &geo, st));
  return (int)hipStreamSynchronize(st);
}

// Input gradient of the critic's second layer through the slab kernel alone (rdgan_d2slab16.hip.h), ndomain 16: gy [B,6,4,4,128],
// the layer's kernel w [3,3,3,64,128] and the gating activation aux [B,11,7,7,64] (layer 1's output) are rounded to bf16 on the
// device; gx [B,11,7,7,64] = conv3d_input_grad(gy, w; stride 2, 'same') * gate(aux) comes back as fp32 (the kernel's bf16 output
// widened).  gate = LeakyReLU'(aux); with use_drop, aux is a stored post-dropout activation (rd_drop_apply: +0.0 = dropped) and
// gate = 0 for dropped elements, LeakyReLU'(aux) / 0.75 for kept ones (rd_gate_from_out).
extern "C" int rdgan_op_d2_dgrad_slab16(const float* gy, const float* w, const float* aux, float* gx, int B, int use_drop, void* stream) {
  if (!gy || !w || !aux || !gx || B < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long nx = (long)B * RD_D2S_OPOS * 64;
  TmpBufs t;
  void* yb = t.to_bf16(gy, (long)B * RD_D2S_SROWS * 128, st);
  void* ab = t.to_bf16(aux, nx, st);
  void* xb = t.bf16(nx);
  void* wi = t.bytes((size_t)RD_D2S_KSTEPS * 2 * 64 * 16);
  RD_TRY(t.rc);
  launch_d2s_wimg(w, wi, st);
  RD_TRY(launch_d2_dgrad_slab(nullptr, kOpRec, yb, wi, ab, xb, B, use_drop != 0, nullptr, st));
  RD_TRY(launch_widen_bf16(xb, gx, nx, st));
  return (int)hipStreamSynchronize(st);
}

// The same through the TILED kernel (k_d2_dgrad_slab_t16): gy [B,6,OH,OW,128], aux / gx [B,11,2 OH - 1,2 OW - 1,64]; OH, OW multiples of 4.
extern "C" int rdgan_op_d2_dgrad_slab_t16(const float* gy, const float* w, const float* aux, float* gx, int B, int OH, int OW, int use_drop,
                                          void* stream) {
  if (!gy || !w || !aux || !gx || B < 1 || OH < 4 || OW < 4 || (OH & 3) || (OW & 3)) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long nx = (long)B * 11 * (2 * OH - 1) * (2 * OW - 1) * 64;
  if (nx * 2 >= 0x7FFFFFF0L) return -2;
  TmpBufs t;
  void* yb = t.to_bf16(gy, (long)B * 6 * OH * OW * 128, st);
  void* ab = t.to_bf16(aux, nx, st);
  void* xb = t.bf16(nx);
  void* wi = t.bytes((size_t)RD_D2S_KSTEPS * 2 * 64 * 16);
  RD_TRY(t.rc);
  RD_TRY((int)hipMemsetAsync(xb, 0xFF, nx * 2, st));          // (NaN pattern: every destination must be written)
  launch_d2s_wimg(w, wi, st);
  RD_TRY(launch_d2_dgrad_slab_t(nullptr, kOpRec, yb, wi, ab, xb, B, OH, OW, use_drop != 0, nullptr, st));
  RD_TRY(launch_widen_bf16(xb, gx, nx, st));
  return (int)hipStreamSynchronize(st);
}

// Generator block 2 forward of the bf16 storage mode through the slab kernel alone (rdgan_upconv16b.hip.h): x [B,6,4,4,256] and the
// Conv3D kernel w [3,3,3,256,128] are rounded to bf16 on the device (the kernel after the upsample collapse), y [B,12,8,8,128] =
// LeakyReLU(PixelNorm(upconv(x) + bias)) comes back as fp32 (the kernel's bf16 output widened), rinv [B,12,8,8].
extern "C" int rdgan_op_upconv2_slab16(const float* x, const float* w, const float* bias, float* y, float* rinv, int B, void* stream) {
  if (!x || !w || !bias || !y || !rinv || B < 1) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long ny = (long)B * 768 * 128;
  TmpBufs t;
  void* xb = t.to_bf16(x, (long)B * 96 * 256, st);
  void* yb = t.bf16(ny);
  void* wi = t.bytes((size_t)RD_UP2_KSTEPS * 4 * 64 * 16);
  float* wc = t.floats(64L * 256 * 128);
  RD_TRY(t.rc);
  hipLaunchKernelGGL(k_collapse_weights, dim3(ew_blocks(16L * 256 * 128)), dim3(256), 0, st, w, wc, 256 * 128);
  launch_upconv2_wimg(wc, wi, st);
  RD_TRY(launch_upconv2_slab(nullptr, kOpRec, xb, wi, bias, yb, rinv, B, st));
  RD_TRY(launch_widen_bf16(yb, y, ny, st));
  return (int)hipStreamSynchronize(st);
}

extern "C" int rdgan_op_pixelnorm_lrelu(const float* y, float* hout, float* rinv, long npix, int C, void* stream) {
  if (!y || !hout) return -2;
  RD_TRY(launch_pn_fwd(nullptr, y, hout, rinv, npix, C, (hipStream_t)stream));
  return (int)hipStreamSynchronize((hipStream_t)stream);
}
extern "C" int rdgan_op_pixelnorm_lrelu_bwd(const float* gh, const float* hh, const float* rinv, float* dy, long npix, int C,
                                            void* stream) {
  if (!gh || !hh || !rinv || !dy) return -2;
  RD_TRY(launch_pn_bwd(nullptr, gh, hh, rinv, dy, npix, C, 0, 0, 0, 0, (hipStream_t)stream));
  return (int)hipStreamSynchronize((hipStream_t)stream);
}

// ---- the step's elementwise kernels one by one (rdgan_elem_launch.h: the launchers the steps use) ----
extern "C" int rdgan_op_softmax_tail(int form, const float* taps, const float* bias, float* out, int* flag, int B, int H, int W,
                                     void* stream) {
  if (!taps || !bias || !out || !flag || B < 1 || H < 1 || W < 1 || (long)B * H * W * RDGAN_NHOURS >= 0x7FFFFFFFL) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (form == 0) launch_colgather_softmax(taps, bias, out, B, H, W, flag, st);
  else if (form == 3 || form == 9) launch_tapsum_softmax_q(form, taps, bias, out, B, H, W, flag, st);
  else if (form == 12 && H == 16 && W == 16) launch_tapsum_softmax12(taps, bias, out, B, flag, st);
  else return -2;
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize(st);
}
extern "C" int rdgan_op_softmax_bwd(const float* p, const float* g, float* dl, int B, int H, int W, void* stream) {
  if (!p || !g || !dl || B < 1 || H < 1 || W < 1 || (long)B * H * W * RDGAN_NHOURS >= 0x7FFFFFFFL) return -2;
  launch_softmax_bwd(p, g, dl, B, H, W, (hipStream_t)stream);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize((hipStream_t)stream);
}
extern "C" int rdgan_op_gp_norm(const float* g0, int B, int per, int CP, int force_S, float* cin_hat_out, float* gp_out, void* stream) {
  if (!g0 || !cin_hat_out || !gp_out || B < 1 || per < 1 || CP < 1 || CP > 4 || force_S < 0 || force_S > 64) return -2;
  if ((long)B * per * CP >= 0x7FFFFFFFL) return -2;
  hipStream_t st = (hipStream_t)stream;
  const int S = force_S ? force_S : gp_norm_slices(B, per);
  TmpBufs t;
  float* part = t.floats((size_t)B * S);
  RD_TRY(t.rc);
  launch_gp_norm(g0, part, cin_hat_out, gp_out, per, B, CP, S, st);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize(st);
}
extern "C" int rdgan_op_loss_tail(int mode, const float* v, const float* gp, int B, int gflag_in, float* out8, void* stream) {
  if (!v || !out8 || B < 1 || (mode != 0 && mode != 1) || (mode == 0 && !gp)) return -2;
  hipStream_t st = (hipStream_t)stream;
  TmpBufs t;
  int* gflag = (int*)t.bytes(sizeof(int));
  RD_TRY(t.rc);
  RD_TRY((int)hipMemcpyAsync(gflag, &gflag_in, sizeof(int), hipMemcpyHostToDevice, st));
  if (mode == 0) launch_critic_losses(v, gp, out8, B, gflag, nullptr, st);
  else launch_gen_loss(v, out8, B, gflag, st);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize(st);
}
extern "C" int rdgan_op_critic_dense(const void* h4, const float* w, const float* bias, float* v_out, void* u4_out, int NB, int F,
                                     int B, int mode, uint64_t seed, int bf16, void* stream) {
  if (!h4 || !w || !bias || !v_out || !u4_out || NB < 1 || F < 1 || B < 1 || (mode != 0 && mode != 1)) return -2;
  if ((long)NB * F >= 0x7FFFFFFFL) return -2;
  hipStream_t st = (hipStream_t)stream;
  launch_critic_dense_fwd(bf16 != 0, h4, w, bias, v_out, NB, F, st);
  launch_critic_top_bwd(bf16 != 0, h4, w, u4_out, NB, F, B, mode, seed, st);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize(st);
}
extern "C" int rdgan_op_critic_dense_wgrad(const void* buf, float* out, int NB, int F, int B, int slices, int bf16, void* stream) {
  if (!buf || !out || NB < 1 || F < 1 || B < 1 || slices < 0 || (long)NB * F >= 0x7FFFFFFFL) return -2;
  hipStream_t st = (hipStream_t)stream;
  const int RS = dense_wgrad_slices(slices, NB);
  TmpBufs t;
  float* part = t.floats((size_t)RS * F);
  RD_TRY(t.rc);
  launch_critic_dense_wgrad(bf16 != 0, buf, out, part, NB, F, B, RS, st);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize(st);
}
extern "C" int rdgan_op_weight_forms(int which, const float* W, float* out, long CC, void* stream) {
  if (!W || !out || CC < 4 || CC % 4 || CC > (1L << 24) || (which != 0 && which != 1)) return -2;
  if (which == 0) launch_collapse_weights(W, out, CC, (hipStream_t)stream);
  else launch_weight_transform(W, out, CC, (hipStream_t)stream);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize((hipStream_t)stream);
}
extern "C" int rdgan_op_weight_forms_adj(int which, const float* dforms, float* dW, long CC, void* stream) {
  if (!dforms || !dW || CC < 4 || CC % 4 || CC > (1L << 24) || (which != 0 && which != 1)) return -2;
  if (which == 0) launch_fold_collapsed_wgrad(dforms, dW, CC, (hipStream_t)stream);
  else launch_weight_transform_adj(dforms, dW, CC, (hipStream_t)stream);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize((hipStream_t)stream);
}
extern "C" int rdgan_op_critic_input(const float* real, const float* fake, const float* cond, float* out, int B, int D, int HW, int nc,
                                     int CP, int mode, uint64_t seed, uint32_t alpha_base, int scalar, void* stream) {
  if (!cond || !out || B < 1 || D < 1 || HW < 1 || nc < 1 || nc > 3 || CP <= nc || CP > 4 || mode < 0 || mode > 2) return -2;
  if ((mode != 1 && !real) || (mode != 2 && !fake)) return -2;
  const long total = (long)B * D * HW;
  if (3 * total * CP >= 0x7FFFFFFFL) return -2;
  launch_critic_input(real, fake, cond, out, B, D, HW, nc, CP, mode, rd_make_key(seed, RD_STREAM_ALPHA), alpha_base,
                      !scalar && critic_input_v4_ok(nc, CP, HW, total), (hipStream_t)stream);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize((hipStream_t)stream);
}
extern "C" int rdgan_op_pool_lrelu_bwd(const float* gup, const float* h0, float* out, int B, int D, int H, int W, int C, void* stream) {
  if (!gup || !h0 || !out || B < 1 || D < 1 || H < 1 || W < 1 || C < 4 || C % 4 || 8L * B * D * H * W * C >= 0x7FFFFFFFL) return -2;
  launch_pool_lrelu_bwd(gup, h0, out, B, D, H, W, C, (hipStream_t)stream);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize((hipStream_t)stream);
}
extern "C" int rdgan_op_lrelu_bwd(const void* g, const void* h, float* out, long n, int bf16, void* stream) {
  if (!g || !h || !out || n < 4 || n % 4) return -2;
  launch_lrelu_bwd(bf16 != 0, g, h, out, n / 4, (hipStream_t)stream);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize((hipStream_t)stream);
}
extern "C" int rdgan_op_colsum(rdgan_handle* h, const void* src, long rows, int C, float* out, int bf16, void* stream) {
  if (!h) return -2;
  if (!src || !out || rows < 1 || C < 1) return bad_arg(h, "op_colsum: bad argument");
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ahead_drain(h, st));
  RD_TRY(launch_colsum(h, (const float*)src, rows, C, out, st, bf16 != 0));
  return (int)hipStreamSynchronize(st);
}
extern "C" int rdgan_op_diff_combine(const void* x, void* E_out, void* dx_inout, const void* dE, int B, int D, long P, int bf16,
                                     void* stream) {
  if (B < 1 || D < 1 || P < 4 || P % 4 || (x == nullptr) != (E_out == nullptr) || (dx_inout == nullptr) != (dE == nullptr)) return -2;
  if (!x && !dx_inout) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (x) launch_diff_d(bf16 != 0, x, E_out, B, D, P, st);
  if (dx_inout) launch_combine_dx(bf16 != 0, dx_inout, dE, B, D, P, st);
  RD_TRY((int)hipGetLastError());
  return (int)hipStreamSynchronize(st);
}

// test hook: the first critic layer's input gradient w.r.t. the sample channel from a given u1 [B][L1][64] (fp32), by the route
// the steps take (critic_input_grad).  with_norm: as the critic step's gradient-penalty sweep does, also leaving gp_out [B] =
// ||g0|| - 1 and cin_hat_out [B][L0][CP] = the second sweep's input.  fp32 storage only.
extern "C" int rdgan_debug_d1_input_grad(rdgan_handle* h, const float* critic_params, const float* u1, int B, int with_norm,
                                         float* g0_out, float* cin_hat_out, float* gp_out, void* stream) {
  if (!h || !critic_params || !u1 || !g0_out) return bad_arg(h, "debug_d1_input_grad: null pointer");
  if (with_norm && (!cin_hat_out || !gp_out)) return bad_arg(h, "debug_d1_input_grad: with_norm needs cin_hat_out and gp_out");
  if (B < 1 || B > h->MB) return bad_arg(h, "debug_d1_input_grad: B outside [1, max_batch]");
  if (h->a16) return bad_arg(h, "debug_d1_input_grad: fp32 storage only");
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ahead_drain(h, st));
  RD_TRY(prep_critic_weights(h, critic_params, st));
  if (with_norm) {
    RD_TRY(critic_penalty_input(h, critic_params, u1, B, h->cin, st));
    RD_CHECK(h, hipMemcpyAsync(cin_hat_out, h->cin, sizeof(float) * B * h->dL[0] * h->CP, hipMemcpyDeviceToDevice, st));
    RD_CHECK(h, hipMemcpyAsync(gp_out, h->gpv, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
  } else
    RD_TRY(critic_input_grad(h, critic_params, u1, B, st));
  RD_CHECK(h, hipMemcpyAsync(g0_out, h->g0, sizeof(float) * B * h->dL[0], hipMemcpyDeviceToDevice, st));
  return 0;
}

// test hook: the activations the last forward left in the workspace (generator h0..h3: which = 0..3, critic layers 1..4
// after LeakyReLU and dropout: which = 4..7), first n floats, as fp32
__global__ void k_bytes_to_f32(const unsigned char* in, float* out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (float)in[i];
}
extern "C" int rdgan_debug_activation(rdgan_handle* h, int which, float* out, long n, void* stream) {
  if (h) RD_TRY(ahead_drain(h, (hipStream_t)stream));
  if (h && out && which == 8 && n >= 1) {      // test hook: layer 1's packed gate bytes (16 per row) as floats
    if (!h->g1bits || n > (long)h->NB * h->dL[1] * 16) return bad_arg(h, "debug_activation: no gate bytes");
    hipLaunchKernelGGL(k_bytes_to_f32, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, h->g1bits, out, n);
    RD_CHECK(h, hipGetLastError());
    return 0;
  }
  if (!h || !out || which < 0 || which > 7 || n < 1) return bad_arg(h, "debug_activation: bad argument");
  const float* src; long cap;
  if (which < 4) {
    float* hs[4] = {h->h0, h->h1, h->h2, h->h3};
    src = hs[which]; cap = (long)h->MB * h->gpix[which] * h->gch[which];
  } else {
    const int l = which - 3;
    src = h->dh[l]; cap = (long)h->NB * h->dL[l] * h->dch[l];
  }
  if (n > cap) return bad_arg(h, "debug_activation: n exceeds the tensor");
  hipStream_t st = (hipStream_t)stream;
  auto copy = [&](const void* from, long first, long cnt) -> int {     // `cnt` elements of `from` -> out[first ..)
    if (cnt <= 0) return 0;
    if (h->a16) {
      hipLaunchKernelGGL(k_bf16_to_f32, dim3(ew_blocks(cnt)), dim3(256), 0, st, (const rd_bf16_t*)from, out + first, cnt);
      RD_CHECK(h, hipGetLastError());
    } else
      RD_CHECK(h, hipMemcpyAsync(out + first, from, sizeof(float) * cnt, hipMemcpyDeviceToDevice, st));
    return 0;
  };
  RD_TRY(copy(src, 0, n));
  if (which >= 4 && h->keep_gates && h->gate_keep_B > 0) {
    // the last call was a critic step: the x_hat third of this layer as it was before the second sweep overwrote it
    const int l = which - 3;
    const long per = h->dL[l] * h->dch[l], first = 2L * h->gate_keep_B * per;
    RD_TRY(copy(h->gate_keep[l], first, std::min<long>(n, first + h->gate_keep_B * per) - first));
  }
  return 0;
}

__global__ void k_rng_probe(uint32_t key, float* mask, float* uni, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (mask) mask[i] = rd_drop_scale(key, (uint32_t)i);
    if (uni) uni[i] = rd_uniform(key, (uint32_t)i);
  }
}
extern "C" int rdgan_op_rng(uint64_t seed, uint32_t stream_id, float* mask_out, float* uniform_out, long n, void* stream) {
  hipLaunchKernelGGL(k_rng_probe, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, rd_make_key(seed, stream_id),
                     mask_out, uniform_out, n);
  return (int)hipStreamSynchronize((hipStream_t)stream);
}

#include "rdgan_eval_entries.h"   // rdgan_data_* ... rdgan_rainfarm_generate: the entry points that take no handle

#ifdef RD_STAMP
extern "C" int rdgan_debug_stamps(unsigned long long* out, int reset) {
  unsigned long long z[8] = {0};
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && out) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(rd_stamp_acc), sizeof(z));
  if (e == hipSuccess && reset) e = hipMemcpyToSymbol(HIP_SYMBOL(rd_stamp_acc), z, sizeof(z));
  return (int)e;
}
extern "C" int rdgan_debug_stamps_ws(unsigned long long* out, int reset) {
  unsigned long long z[8] = {0};
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && out) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(rd_stamp_ws), sizeof(z));
  if (e == hipSuccess && reset) e = hipMemcpyToSymbol(HIP_SYMBOL(rd_stamp_ws), z, sizeof(z));
  return (int)e;
}
#endif
