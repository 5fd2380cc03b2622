// The handle-free entry points of include/rdgan.h: input pipeline, CRPS experiment, distribution checks, whole fields, ensemble
// products, verification, the evaluations of hourly arrays (temporal structure, rain cells, storms, areal extremes, catchment
// rainfall, space-time structure), analogs, seams between days, scenario reduction, spectra and RainFARM.  They take no rdgan_handle and use nothing of the step engine but RD_TRY,
// ensure_lds(nullptr, ...) and ew_blocks.  Host code, included by rdgan_api.hip at one point, behind the op-level test entries (the
// library stays one translation unit: one code object for the ISA lint).
//
// An *_accumulate entry of an hourly evaluation admits its array with rd_hourly_layout_ok and sizes its passes with rd_pass_units
// (rdgan_hourly_host.h, host-only, tested on its own); the pass loop and its launches are the entry's own.
#pragma once
#include "rdgan_hourly_host.h"

static int rd_pow2_at_least(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// the tables of a DFT of length nd: re[j] + i im[j] = exp(sign * 2 pi i j / nd), computed in fp64 and rounded once to T
template <typename T>
static void rd_twiddles(int nd, double sign, T* re, T* im) {
  for (int j = 0; j < nd; ++j) {
    const double th = sign * 2.0 * M_PI * (double)j / (double)nd;
    re[j] = (T)cos(th);
    im[j] = (T)sin(th);
  }
}

// ------------------------------------------------------------------------------------
// input pipeline
// ------------------------------------------------------------------------------------
extern "C" int rdgan_data_gather(const float* data, int n_days, int ny, int nx, const int* indices, int n, int ndomain,
                                 float norm_scale, float* batch_out, float* cond_out, int* flags, void* stream) {
  if (!data || !indices || !cond_out || !flags || n_days < 1 || n < 1 || ndomain < 1 || ndomain > ny || ndomain > nx) return -2;
  // *flags accumulates over calls (include/rdgan.h): the caller zeroes it before the first gather and after reading it
  hipLaunchKernelGGL(k_gather_tiles, dim3(ew_blocks((long)n * ndomain * ndomain)), dim3(256), 0, (hipStream_t)stream, data, n_days,
                     RDGAN_NHOURS, ny, nx, indices, n, ndomain, norm_scale, batch_out, cond_out, flags);
  return (int)hipGetLastError();
}

extern "C" int rdgan_data_valid_tiles(const float* data, int n_days, int ny, int nx, int ndomain, int stride,
                                      float tp_thresh_daily, int n_thresh, int* valid_out, void* stream) {
  if (!data || !valid_out || n_days < 1 || ny < 1 || nx < 1 || stride < 1 || ndomain < 1 || ndomain > ny || ndomain > nx) return -2;
  const int nbi = (ny - ndomain + stride - 1) / stride, nbj = (nx - ndomain + stride - 1) / stride;   // len(range(0, ny-nd, stride))
  if (nbi < 1 || nbj < 1) return 0;
  const long blocks = (long)n_days * nbi * nbj;
  if (blocks > 0xFFFFFFL) return -2;       // one 256-thread block per box and no loop: a launch holds fewer than 2^32 threads
  hipLaunchKernelGGL(k_valid_tiles, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, data, RDGAN_NHOURS, ny, nx,
                     ndomain, stride, nbi, nbj, tp_thresh_daily, n_thresh, valid_out);
  return (int)hipGetLastError();
}

// training set from raw radar frames (rdgan_radar.hip.h)
template <int W, int FPH>
static void launch_radar_hourly(const unsigned char* codes, const float* lut, long n_days, long plane, float* hourly, float* daily,
                                unsigned long long* missing, hipStream_t st) {
  const long groups = (plane + W - 1) / W;
  // (a launch holds fewer than 2^32 threads; the kernel's grid-stride loop takes what lies beyond)
  const long blocks = std::min<long>((n_days * groups + RD_RADAR_THREADS - 1) / RD_RADAR_THREADS, 0xFFFFFFL);
  hipLaunchKernelGGL((k_radar_hourly<W, FPH>), dim3((unsigned)blocks), dim3(RD_RADAR_THREADS), 0, st, codes, lut, n_days, plane, groups,
                     hourly, daily, missing);
}
template <int W>
static void launch_radar_hourly_w(int fph, const unsigned char* codes, const float* lut, long n_days, long plane, float* hourly,
                                  float* daily, unsigned long long* missing, hipStream_t st) {
  switch (fph) {
    case 1: launch_radar_hourly<W, 1>(codes, lut, n_days, plane, hourly, daily, missing, st); break;
    case 2: launch_radar_hourly<W, 2>(codes, lut, n_days, plane, hourly, daily, missing, st); break;
    case 3: launch_radar_hourly<W, 3>(codes, lut, n_days, plane, hourly, daily, missing, st); break;
    case 4: launch_radar_hourly<W, 4>(codes, lut, n_days, plane, hourly, daily, missing, st); break;
    case 6: launch_radar_hourly<W, 6>(codes, lut, n_days, plane, hourly, daily, missing, st); break;
    default: launch_radar_hourly<W, 12>(codes, lut, n_days, plane, hourly, daily, missing, st); break;
  }
}

extern "C" int rdgan_data_radar_hourly(const unsigned char* codes, const float* lut256, long n_days, int frames_per_hour, int ny, int nx,
                                       float* hourly_out, float* daily_out, unsigned long long* missing_out, void* stream) {
  const int f = frames_per_hour;
  if (!codes || !lut256 || !hourly_out || n_days < 1 || ny < 1 || nx < 1) return -2;
  if (f != 1 && f != 2 && f != 3 && f != 4 && f != 6 && f != 12) return -2;
  const long plane = (long)ny * nx;
  hipStream_t st = (hipStream_t)stream;
  // 16 codes per lane: every frame and every output row group starts on a 16-byte boundary; 4 per lane: dword loads, float4 stores
  const uintptr_t out_bits = (uintptr_t)hourly_out | (uintptr_t)daily_out;
  if (plane % 16 == 0 && (((uintptr_t)codes | out_bits) & 15) == 0)
    launch_radar_hourly_w<16>(f, codes, lut256, n_days, plane, hourly_out, daily_out, missing_out, st);
  else if (plane % 4 == 0 && ((uintptr_t)codes & 3) == 0 && (out_bits & 15) == 0)
    launch_radar_hourly_w<4>(f, codes, lut256, n_days, plane, hourly_out, daily_out, missing_out, st);
  else
    launch_radar_hourly_w<1>(f, codes, lut256, n_days, plane, hourly_out, daily_out, missing_out, st);
  return (int)hipGetLastError();
}

extern "C" int rdgan_data_daily_sum(const float* hourly, long n_days, int ny, int nx, float* daily_out, void* stream) {
  if (!hourly || !daily_out || n_days < 1 || ny < 1 || nx < 1) return -2;
  const long plane = (long)ny * nx;
  hipLaunchKernelGGL(k_daily_sum, dim3(ew_blocks(n_days * plane)), dim3(256), 0, (hipStream_t)stream, hourly, n_days, plane, daily_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_data_valid_tiles_daily(const float* daily, long n_days, int ny, int nx, int ndomain, int stride,
                                            float tp_thresh_daily, int n_thresh, int* valid_out, void* stream) {
  if (!daily || !valid_out || n_days < 1 || ny < 1 || nx < 1 || stride < 1 || ndomain < 1 || ndomain > ny || ndomain > nx) return -2;
  const int nbi = (ny - ndomain + stride - 1) / stride, nbj = (nx - ndomain + stride - 1) / stride;   // len(range(0, ny-nd, stride))
  if (nbi < 1 || nbj < 1) return 0;
  const long boxes = n_days * nbi * nbj;
  const long blocks = std::min<long>((boxes + 3) / 4, 0xFFFFFFL);      // fewer than 2^32 threads per launch; the kernel loops over the rest
  hipLaunchKernelGGL(k_valid_tiles_daily, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, daily, boxes, ny, nx, ndomain,
                     stride, nbi, nbj, tp_thresh_daily, n_thresh, valid_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_crps_ensemble(const float* ens, const float* obs, const float* scale, float* crps_out, int n,
                                   long npix, void* stream) {
  if (!ens || !obs || !crps_out || n < 1 || n > 8192 || npix < 1 || npix > 0x7FFFFFFFL) return -2;
  const int npow2 = rd_pow2_at_least(n);
  hipLaunchKernelGGL(k_crps_ensemble, dim3((unsigned)npix), dim3(256), npow2 * sizeof(float), (hipStream_t)stream, ens, obs,
                     scale, crps_out, n, npow2, npix);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// CRPS experiment (rdgan_crps.hip.h): fixed-ensemble CRPS, bootstrapped means, moments
// ------------------------------------------------------------------------------------
extern "C" int rdgan_crps_fixed_ensemble(const float* ens, const float* obs, float* crps_out, float* hourly_out, int n,
                                         long n_days, int nd, void* stream) {
  if (!ens || !obs || (!crps_out && !hourly_out) || n < 1 || n > RD_CRPS_MAXN || n_days < 1 || nd < 1 || nd > 1024) return -2;
  const long npos = (long)RDGAN_NHOURS * nd * nd;
  if (npos > 0x7FFFFFFFL || n_days > 0x7FFFFFFFL / npos) return -2;       // D * npos < 2^31, and the grids below fit
  hipStream_t st = (hipStream_t)stream;
  const int npow2 = rd_pow2_at_least(n);
  const size_t lds = (size_t)(n + 1 + RD_CRPS_THREADS) * sizeof(double) + (size_t)npow2 * sizeof(float);
  RD_TRY(ensure_lds(nullptr, (const void*)k_crps_fixed, lds));
  // the hourly means are taken over the per-position values: without a caller's buffer they live in a stream-ordered temporary
  float* per_pos = crps_out;
  if (!per_pos) {
    hipError_t e = hipMallocAsync((void**)&per_pos, (size_t)n_days * npos * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_crps_fixed, dim3((unsigned)npos), dim3(RD_CRPS_THREADS), lds, st, ens, obs, per_pos, n, npow2, n_days, npos);
  if (hourly_out)
    hipLaunchKernelGGL(k_crps_hourly, dim3((unsigned)(n_days * RDGAN_NHOURS)), dim3(256), 0, st, per_pos, hourly_out, nd * nd);
  hipError_t e = hipGetLastError();
  if (!crps_out) {
    hipError_t f = hipFreeAsync(per_pos, st);
    if (e == hipSuccess) e = f;
  }
  return (int)e;
}

extern "C" int rdgan_bootstrap_means(const double* x, long n, uint64_t seed, long first_resample, long n_resamples,
                                     double* means_out, void* stream) {
  if (!x || !means_out || n < 1 || n > 0xFFFFFFFFL || first_resample < 0 || n_resamples < 1 || n_resamples > 0x7FFFFFFFL) return -2;
  hipLaunchKernelGGL(k_bootstrap_means, dim3((unsigned)n_resamples), dim3(RD_CRPS_THREADS), 0, (hipStream_t)stream, x, (uint32_t)n,
                     rd_make_key(seed, RD_STREAM_BOOTSTRAP), (uint64_t)first_resample, means_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_moments_f64(const double* x, long n, double* out3, void* stream) {
  if (!x || !out3 || n < 1) return -2;
  hipLaunchKernelGGL(k_moments_f64, dim3(1), dim3(RD_CRPS_THREADS), 0, (hipStream_t)stream, x, n, out3);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// distribution checks (rdgan_dist.hip.h): two-sample KS, box-plot statistics, ECDF on a grid
// ------------------------------------------------------------------------------------
extern "C" int rdgan_ks_2samp(const float* a, const float* b, int n, int m, int ncol, long batch, int* counts_out, double* d_out,
                              void* stream) {
  if (!a || !b || !counts_out || !d_out || n < 1 || n > RD_DIST_MAXN || m < 1 || m > RD_DIST_MAXN || ncol < 1 || batch < 1) return -2;
  if (batch > 0x7FFFFFFFL / ncol) return -2;
  const int npa = rd_pow2_at_least(n), npb = rd_pow2_at_least(m);
  RD_TRY(ensure_lds(nullptr, (const void*)k_ks_2samp, RD_KS_LDS_MAX));
  hipLaunchKernelGGL(k_ks_2samp, dim3((unsigned)(batch * ncol)), dim3(RD_DIST_THREADS),
                     RD_KS_LDS_HEAD + (size_t)(npa + npb) * sizeof(float), (hipStream_t)stream, a, b, n, m, npa, npb, ncol, counts_out,
                     d_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_box_stats(const float* x, int n, int ncol, long batch, double* stats_out, float* sorted_out, void* stream) {
  if (!x || !stats_out || n < 1 || n > RD_DIST_MAXN || ncol < 1 || batch < 1) return -2;
  if (batch > 0x7FFFFFFFL / ncol) return -2;
  const int npow2 = rd_pow2_at_least(n);
  RD_TRY(ensure_lds(nullptr, (const void*)k_box_stats, RD_BOX_LDS_MAX));
  hipLaunchKernelGGL(k_box_stats, dim3((unsigned)(batch * ncol)), dim3(RD_DIST_THREADS), RD_BOX_LDS_HEAD + (size_t)npow2 * sizeof(float),
                     (hipStream_t)stream, x, n, npow2, ncol, stats_out, sorted_out);
  return (int)hipGetLastError();
}

extern "C" long rdgan_ecdf_workspace_bytes(int n_grid) {
  if (n_grid < 1 || n_grid > RD_ECDF_MAXT) return -2;
  return (long)(n_grid + 2) * (long)sizeof(unsigned long long);
}

extern "C" int rdgan_ecdf_grid(const float* x, long n_values, const float* grid, int n_grid, long long* counts_out, void* workspace,
                               long workspace_bytes, void* stream) {
  if (!x || !grid || !counts_out || !workspace || n_values < 1 || n_values > (1L << 40) || n_grid < 1 || n_grid > RD_ECDF_MAXT) return -2;
  if (((unsigned long long)x & 3) || workspace_bytes < rdgan_ecdf_workspace_bytes(n_grid)) return -2;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* hist = (unsigned long long*)workspace;
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)(n_grid + 2) * sizeof(unsigned long long), st);
  if (e != hipSuccess) return (int)e;
  const long per_block = (long)RD_ECDF_THREADS * 16;                     // four float4 per thread
  const long blocks = std::max<long>(1, std::min<long>(RD_ECDF_MAXBLOCKS, (n_values + per_block - 1) / per_block));
  hipLaunchKernelGGL(k_ecdf_grid, dim3((unsigned)blocks), dim3(RD_ECDF_THREADS), (size_t)(2 * n_grid + 2) * sizeof(float), st, x,
                     n_values, grid, n_grid, hist);
  hipLaunchKernelGGL(k_ecdf_scan, dim3(1), dim3(RD_DIST_THREADS), 0, st, hist, n_grid, counts_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// whole daily fields (rdgan_field.hip.h): tile scan, condition batch, blend
// ------------------------------------------------------------------------------------
static bool rd_field_geometry_ok(long n_days, int ny, int nx, int nd, int overlap) {
  return rd_geometry_ok(nd, 1, 1) && overlap >= 0 && overlap <= nd / 2 && ny >= nd && nx >= nd && n_days >= 1;
}

// a small host table for the next launch: a stream-ordered device copy, freed behind the launch by the caller
static int rd_field_upload(const int* host, size_t n, int** dev, hipStream_t st) {
  hipError_t e = hipMallocAsync((void**)dev, n * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(*dev, host, n * sizeof(int), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    (void)hipFreeAsync(*dev, st);
    return (int)e;
  }
  return 0;
}

extern "C" int rdgan_field_scan(const float* daily, long n_days, int ny, int nx, int nd, int overlap, int* counts_out, void* stream) {
  if (!daily || !counts_out || !rd_field_geometry_ok(n_days, ny, nx, nd, overlap)) return -2;
  const int step = nd - overlap, n_ty = rd_field_axis_tiles(ny, nd, step), n_tx = rd_field_axis_tiles(nx, nd, step);
  if ((long)n_ty * n_tx > 0x7FFFFFFFL / n_days) return -2;                 // an entry number day * T + tile is an int32
  const long entries = n_days * n_ty * n_tx;
  const long blocks = std::min<long>((entries + 3) / 4, 0xFFFFFFL);        // the kernel loops over the rest
  hipLaunchKernelGGL(k_field_scan, dim3((unsigned)blocks), dim3(RD_FIELD_THREADS), 0, (hipStream_t)stream, daily, entries, ny, nx, nd,
                     step, n_ty, n_tx, counts_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_field_cond(const float* daily, long n_days, int ny, int nx, int nd, int overlap, const int* entries, long m,
                                double norm_scale, float* cond_out, void* stream) {
  if (!daily || !entries || !cond_out || m < 1 || !(norm_scale > 0.0) || !rd_field_geometry_ok(n_days, ny, nx, nd, overlap)) return -2;
  const int step = nd - overlap, n_ty = rd_field_axis_tiles(ny, nd, step), n_tx = rd_field_axis_tiles(nx, nd, step);
  if ((long)n_ty * n_tx > 0x7FFFFFFFL / n_days) return -2;
  const long n_entries = n_days * n_ty * n_tx;
  for (long i = 0; i < m; ++i)
    if (entries[i] < 0 || entries[i] >= n_entries) return -2;
  hipStream_t st = (hipStream_t)stream;
  int* dev = nullptr;
  RD_TRY(rd_field_upload(entries, (size_t)m, &dev, st));
  hipLaunchKernelGGL(k_field_cond, dim3(ew_blocks(m * nd * nd, RD_FIELD_THREADS)), dim3(RD_FIELD_THREADS), 0, st, daily, dev, m, ny, nx,
                     nd, step, n_ty, n_tx, norm_scale, cond_out);
  hipError_t e = hipGetLastError();
  hipError_t f = hipFreeAsync(dev, st);
  return (int)(e != hipSuccess ? e : f);
}

// What the two blend entries share: the slot table of `units` units checked against m and the geometry, and uploaded for the launch
struct rd_blend_plan {
  int* dev;                 // the slot table on the device: rd_blend_done frees it behind the launch
  int step, n_ty, n_tx;
  long nb;                  // pixel blocks of all units
};

// the caller has checked its pointers; -2 for a bad size, geometry or slot, otherwise the upload's code
static int rd_blend_slots(long m, const int* slots, long units, long first_unit, long n_days, int ny, int nx, int nd, int overlap,
                          hipStream_t st, rd_blend_plan* p) {
  if (m < 1 || m > 0x7FFFFFFFL || units < 1 || first_unit < 0 || !rd_field_geometry_ok(n_days, ny, nx, nd, overlap)) return -2;
  p->step = nd - overlap, p->n_ty = rd_field_axis_tiles(ny, nd, p->step), p->n_tx = rd_field_axis_tiles(nx, nd, p->step);
  const long T = (long)p->n_ty * p->n_tx;
  if (T > 0x7FFFFFFFL || units > 0x7FFFFFFFL / T) return -2;
  for (long i = 0; i < units * T; ++i)
    if (slots[i] < -1 || slots[i] >= m) return -2;
  p->nb = units * ((ny + RD_FIELD_BY - 1) / RD_FIELD_BY) * ((nx + RD_FIELD_BX - 1) / RD_FIELD_BX);
  p->dev = nullptr;
  return rd_field_upload(slots, (size_t)(units * T), &p->dev, st);
}

// behind the blend launch: its error, or else the error of freeing the table (the first error wins)
static int rd_blend_done(const rd_blend_plan& p, hipStream_t st) {
  hipError_t e = hipGetLastError();
  hipError_t f = hipFreeAsync(p.dev, st);
  return (int)(e != hipSuccess ? e : f);
}

extern "C" int rdgan_field_blend(const float* frac, long m, const int* slots, long units, long first_unit, const int* ytab_idx,
                                 const float* ytab_w, const int* xtab_idx, const float* xtab_w, const float* daily, long n_days,
                                 int ny, int nx, int nd, int overlap, float* out, void* stream) {
  if (!frac || !slots || !ytab_idx || !ytab_w || !xtab_idx || !xtab_w || !daily || !out) return -2;
  hipStream_t st = (hipStream_t)stream;
  rd_blend_plan p;
  RD_TRY(rd_blend_slots(m, slots, units, first_unit, n_days, ny, nx, nd, overlap, st, &p));
  hipLaunchKernelGGL(k_field_blend, dim3((unsigned)std::min<long>(p.nb, 1L << 20)), dim3(RD_FIELD_THREADS), 0, st, frac, p.dev, ytab_idx,
                     ytab_w, xtab_idx, xtab_w, daily, out, units, first_unit, n_days, ny, nx, nd, p.step, p.n_ty, p.n_tx);
  return rd_blend_done(p, st);
}

// ------------------------------------------------------------------------------------
// ensemble products (rdgan_products.hip.h): k-hour peaks of hourly maps, the blend fused with them, member statistics
// ------------------------------------------------------------------------------------
// the window list as the kernels take it: bit w - 1 set for every window w; false for a list that is not strictly increasing in 1 .. 24
static bool rd_peaks_mask(const int* windows, int n_windows, unsigned* mask) {
  if (!windows || n_windows < 1 || n_windows > RD_PEAKS_MAXK) return false;
  unsigned m = 0;
  for (int i = 0; i < n_windows; ++i) {
    if (windows[i] < 1 || windows[i] > RD_HOURS || (i > 0 && windows[i] <= windows[i - 1])) return false;
    m |= 1u << (windows[i] - 1);
  }
  *mask = m;
  return true;
}

extern "C" int rdgan_hourly_peaks(const float* hourly, long units, int ny, int nx, const int* windows, int n_windows, float* peaks_out,
                                  unsigned char* peak_hour_out, void* stream) {
  unsigned mask = 0;
  if (!hourly || !peaks_out || !peak_hour_out || units < 1 || ny < 1 || nx < 1 || !rd_peaks_mask(windows, n_windows, &mask)) return -2;
  const long nb = ((ny + RD_FIELD_BY - 1) / RD_FIELD_BY) * (long)((nx + RD_FIELD_BX - 1) / RD_FIELD_BX);
  if (units > (1L << 40) / nb) return -2;
  hipLaunchKernelGGL(k_hourly_peaks, dim3((unsigned)std::min<long>(units * nb, 1L << 20)), dim3(RD_FIELD_THREADS), 0,
                     (hipStream_t)stream, hourly, units, ny, nx, mask, windows[0], peaks_out, peak_hour_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_field_blend_peaks(const float* frac, long m, const int* slots, long units, long first_unit, const int* ytab_idx,
                                       const float* ytab_w, const int* xtab_idx, const float* xtab_w, const float* daily, long n_days,
                                       int ny, int nx, int nd, int overlap, const int* windows, int n_windows, float* peaks_out,
                                       unsigned char* peak_hour_out, void* stream) {
  unsigned mask = 0;
  if (!frac || !slots || !ytab_idx || !ytab_w || !xtab_idx || !xtab_w || !daily || !peaks_out || !peak_hour_out) return -2;
  if (!rd_peaks_mask(windows, n_windows, &mask)) return -2;
  hipStream_t st = (hipStream_t)stream;
  rd_blend_plan p;
  RD_TRY(rd_blend_slots(m, slots, units, first_unit, n_days, ny, nx, nd, overlap, st, &p));
  hipLaunchKernelGGL(k_field_blend_peaks, dim3((unsigned)std::min<long>(p.nb, 1L << 20)), dim3(RD_FIELD_THREADS), 0, st, frac, p.dev,
                     ytab_idx, ytab_w, xtab_idx, xtab_w, daily, peaks_out, peak_hour_out, units, first_unit, n_days, ny, nx, nd, p.step,
                     p.n_ty, p.n_tx, mask, windows[0]);
  return rd_blend_done(p, st);
}

extern "C" int rdgan_member_stats(const float* x, int n_members, long member_stride, long n_positions, const double* probs, int n_probs,
                                  const double* thresholds, int n_thresholds, float* quantiles_out, float* mean_out, float* exceed_out,
                                  long long* n_nan_positions_out, void* stream) {
  if (!x || !probs || !quantiles_out || !mean_out || !n_nan_positions_out) return -2;
  if (n_members < 1 || n_members > RD_MS_MAXS || n_positions < 1 || n_positions > (1L << 40) || member_stride < n_positions) return -2;
  if (n_probs < 1 || n_probs > RD_MS_MAXQ || n_thresholds < 0 || n_thresholds > RD_MS_MAXT) return -2;
  if (n_thresholds > 0 && (!thresholds || !exceed_out)) return -2;
  rd_ms_args a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_probs; ++i) {
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return -2;
    a.probs[i] = probs[i];
  }
  for (int i = 0; i < n_thresholds; ++i) {
    if (!std::isfinite(thresholds[i])) return -2;
    a.thr[i] = thresholds[i];
  }
  const int np2 = rd_pow2_at_least(n_members);
  const int px = rd_ms_run_width(np2);
  int lpx = 0;
  while ((1 << lpx) < px) ++lpx;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ensure_lds(nullptr, (const void*)k_member_stats, RD_MS_LDS_MAX));
  hipError_t e = hipMemsetAsync(n_nan_positions_out, 0, sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  const long runs = (n_positions + px - 1) / px;
  hipLaunchKernelGGL(k_member_stats, dim3((unsigned)std::min<long>(runs, 1L << 16)), dim3(RD_MS_THREADS),
                     RD_MS_LDS_HEAD + (size_t)np2 * px * sizeof(float), st, x, member_stride, n_members, np2, lpx, n_positions, n_probs,
                     n_thresholds, a, quantiles_out, mean_out, exceed_out, (unsigned long long*)n_nan_positions_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// verification of field ensembles (rdgan_verify.hip.h): state accumulation, rank / reliability / Brier reduction, FSS
// ------------------------------------------------------------------------------------
// the thresholds as the kernels compare them: each rounded once to fp32; false unless finite, >= 0 and strictly increasing there
static bool rd_thresholds(const double* thresholds, int n, rd_thr* out) {
  if (!thresholds || n < 1 || n > RD_THR_MAX) return false;
  memset(out, 0, sizeof(*out));
  for (int i = 0; i < n; ++i) {
    if (!(thresholds[i] >= 0.0 && thresholds[i] <= 3.4028234663852886e38)) return false;        // (a NaN fails both)
    const float f = (float)thresholds[i];
    if (i > 0 && !(f > out->v[i - 1])) return false;
    out->v[i] = f;
  }
  return true;
}

static bool rd_vf_widths_ok(const int* widths, int n, int S, rd_vf_widths* out) {
  if (!widths || n < 1 || n > RD_VF_MAXW) return false;
  memset(out, 0, sizeof(*out));
  for (int i = 0; i < n; ++i) {
    if (widths[i] < 1 || widths[i] % 2 == 0 || (i > 0 && widths[i] <= widths[i - 1])) return false;
    if (widths[i] > 8192 || (long)S * widths[i] * widths[i] >= (1L << 26)) return false;
    out->v[i] = widths[i];
  }
  return true;
}

template <int V>
static void rd_vf_launch_accumulate(int T, unsigned blocks, hipStream_t st, const float* x, long stride, int n, long P, const float* obs,
                                    const rd_thr& thr, int* exceed, int* below, int* equal, unsigned char* bad) {
#define RD_VF_CASE(TT)                                                                                                              \
  case TT:                                                                                                                          \
    hipLaunchKernelGGL((k_verify_accumulate<TT, V>), dim3(blocks), dim3(RD_VF_THREADS), 0, st, x, stride, n, P, obs, thr, exceed,    \
                       below, equal, bad);                                                                                          \
    break;
  switch (T) {
    RD_VF_CASE(1) RD_VF_CASE(2) RD_VF_CASE(3) RD_VF_CASE(4) RD_VF_CASE(5) RD_VF_CASE(6) RD_VF_CASE(7) RD_VF_CASE(8)
  }
#undef RD_VF_CASE
}

extern "C" int rdgan_verify_accumulate(const float* members, int n_members, long member_stride, long n_positions, const float* obs,
                                       const double* thresholds, int n_thresholds, int* exceed, int* below, int* equal,
                                       unsigned char* bad, void* stream) {
  rd_thr thr;
  if (!members || !obs || !exceed || !below || !equal || !bad) return -2;
  if (n_members < 1 || n_members > RD_VF_MAXS || n_positions < 1 || n_positions > (1L << 40) || member_stride < n_positions) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  const unsigned long long align = (unsigned long long)members | (unsigned long long)obs | (unsigned long long)exceed |
                                   (unsigned long long)below | (unsigned long long)equal;
  if (align & 3) return -2;
  // 16-byte loads where every row of every array starts on 16 bytes: the member rows (base and stride), the T planes of exceed (P)
  const bool vec = !(align & 15) && !((unsigned long long)bad & 3) && member_stride % 4 == 0 && n_positions % 4 == 0;
  const long groups = vec ? n_positions / 4 : n_positions;
  const unsigned blocks = (unsigned)std::min<long>((groups + RD_VF_THREADS - 1) / RD_VF_THREADS, 1L << 16);
  if (vec)
    rd_vf_launch_accumulate<4>(n_thresholds, blocks, (hipStream_t)stream, members, member_stride, n_members, n_positions, obs, thr,
                               exceed, below, equal, bad);
  else
    rd_vf_launch_accumulate<1>(n_thresholds, blocks, (hipStream_t)stream, members, member_stride, n_members, n_positions, obs, thr,
                               exceed, below, equal, bad);
  return (int)hipGetLastError();
}

extern "C" int rdgan_verify_reduce(const float* obs, const int* exceed, const int* below, const int* equal, const unsigned char* bad,
                                   long n_positions, long plane, int n_members, const double* thresholds, int n_thresholds, int n_bins,
                                   uint64_t seed, long long* rank_hist_out, long long* reliability_out, long long* brier_out,
                                   void* stream) {
  rd_thr thr;
  if (!obs || !exceed || !below || !equal || !bad || !rank_hist_out || !reliability_out || !brier_out) return -2;
  if (n_members < 1 || n_members > RD_VF_MAXS || n_bins < 2 || n_bins > std::min(n_members + 1, RD_VF_MAXBINS)) return -2;
  if (plane < 1 || n_positions < 1 || n_positions > (1L << 40) || n_positions % plane) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  const int S = n_members, T = n_thresholds;
  const long n_planes = n_positions / plane;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(rank_hist_out, 0, (size_t)RD_HOURS * (S + 1) * sizeof(long long), st);
  if (e == hipSuccess) e = hipMemsetAsync(reliability_out, 0, (size_t)T * RD_HOURS * n_bins * 3 * sizeof(long long), st);
  if (e == hipSuccess) e = hipMemsetAsync(brier_out, 0, (size_t)T * RD_HOURS * 4 * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  const long units = ((n_planes + RD_HOURS - 1) / RD_HOURS) * ((plane + RD_VF_CHUNK - 1) / RD_VF_CHUNK);       // per hour
  // at most RD_VF_MAXUNITS chunks per workgroup (the 32-bit LDS counters), at least 64 workgroups per hour where there is work
  const long nbx = std::max<long>((units + RD_VF_MAXUNITS - 1) / RD_VF_MAXUNITS, std::min<long>(units, 64));
  const size_t lds = RD_VF_MAXT * 4 * sizeof(unsigned long long) + (size_t)(T * n_bins * 3 + S + 1) * sizeof(unsigned);
  hipLaunchKernelGGL(k_verify_reduce, dim3((unsigned)nbx, RD_HOURS), dim3(RD_VF_THREADS), lds, st, obs, exceed, below, equal, bad,
                     n_positions, plane, n_planes, S, T, thr, n_bins, rd_make_key(seed, RD_STREAM_VERIFY),
                     (unsigned long long*)rank_hist_out, (unsigned long long*)reliability_out, (unsigned long long*)brier_out);
  return (int)hipGetLastError();
}

static long rd_vf_box_blocks(long plane) { return std::min<long>((plane + RD_VF_THREADS - 1) / RD_VF_THREADS, RD_VF_BOX_MAXBLOCKS); }

extern "C" long rdgan_verify_fss_workspace_bytes(int ny, int nx, int n_thresholds, int n_widths) {
  if (ny < 1 || nx < 1 || n_thresholds < 1 || n_thresholds > RD_VF_MAXT || n_widths < 1 || n_widths > RD_VF_MAXW) return -2;
  const long plane = (long)ny * nx, planes = (long)RD_HOURS * n_thresholds;
  if (plane > (1L << 36)) return -2;
  return planes * rd_vf_box_blocks(plane) * n_widths * 2 * (long)sizeof(double) + 2 * planes * plane * (long)sizeof(unsigned);
}

extern "C" int rdgan_verify_fss(const float* obs, const int* exceed, const unsigned char* bad, long n_days, int ny, int nx,
                                int n_members, const double* thresholds, int n_thresholds, const int* widths, int n_widths,
                                double* fss_sums_out, void* workspace, long workspace_bytes, void* stream) {
  rd_thr thr;
  rd_vf_widths wd;
  if (!obs || !exceed || !bad || !fss_sums_out || !workspace || ((unsigned long long)workspace & 7)) return -2;
  if (n_days < 1 || ny < 1 || nx < 1 || n_members < 1 || n_members > RD_VF_MAXS) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr) || !rd_vf_widths_ok(widths, n_widths, n_members, &wd)) return -2;
  const long need = rdgan_verify_fss_workspace_bytes(ny, nx, n_thresholds, n_widths);
  if (need < 0 || workspace_bytes < need) return -2;
  const int T = n_thresholds, W = n_widths;
  const long plane = (long)ny * nx, planes = (long)RD_HOURS * T;
  if (n_days > (1L << 40) / (plane * RD_HOURS)) return -2;
  const long P = n_days * RD_HOURS * plane, rows = planes * ny, cols = planes * nx;
  if ((rows + 3) / 4 > 0x7FFFFFFFL || (cols + RD_VF_THREADS - 1) / RD_VF_THREADS > 0x7FFFFFFFL) return -2;
  const int nblk = (int)rd_vf_box_blocks(plane);
  double* partial = (double*)workspace;
  unsigned* satC = (unsigned*)(partial + planes * nblk * W * 2);
  unsigned* satE = satC + planes * plane;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(fss_sums_out, 0, (size_t)T * W * RD_HOURS * 2 * sizeof(double), st);
  if (e != hipSuccess) return (int)e;
  for (long day = 0; day < n_days; ++day) {                 // the days one after another: the workspace holds one day's tables
    hipLaunchKernelGGL(k_verify_fss_rows, dim3((unsigned)((rows + 3) / 4)), dim3(RD_VF_THREADS), 0, st, obs, exceed, bad, P, day, ny, nx,
                       n_members, T, thr, satC, satE);
    hipLaunchKernelGGL(k_verify_fss_cols, dim3((unsigned)((cols + RD_VF_THREADS - 1) / RD_VF_THREADS)), dim3(RD_VF_THREADS), 0, st, satC,
                       satE, planes, ny, nx);
    hipLaunchKernelGGL(k_verify_fss_box, dim3((unsigned)nblk, (unsigned)planes), dim3(RD_VF_THREADS), 0, st, satC, satE, ny, nx,
                       n_members, wd, W, partial);
    hipLaunchKernelGGL(k_verify_fss_final, dim3((unsigned)((planes * W + RD_VF_THREADS - 1) / RD_VF_THREADS)), dim3(RD_VF_THREADS), 0,
                       st, partial, nblk, T, W, fss_sums_out);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// temporal structure of hourly fields (rdgan_temporal.hip.h): spells, transitions, wet hours, lagged products
// ------------------------------------------------------------------------------------
// workgroups of k_temporal_accumulate for `groups` threads' worth of work
static long rd_ts_blocks(long groups) { return std::min<long>((groups + RD_TS_THREADS - 1) / RD_TS_THREADS, RD_TS_MAXBLOCKS); }

static bool rd_ts_shape_ok(long n, long plane, int n_thresholds, int max_lag) {
  if (n < 1 || plane < 1 || n_thresholds < 1 || n_thresholds > RD_TS_MAXT || max_lag < 1 || max_lag > RD_TS_MAXK) return false;
  return plane <= RD_HOURLY_MAXELEMS / RD_HOURS && n <= RD_HOURLY_MAXELEMS / (RD_HOURS * plane);
}

extern "C" long rdgan_temporal_workspace_bytes(long n, long plane, int n_thresholds, int max_lag) {
  if (!rd_ts_shape_ok(n, plane, n_thresholds, max_lag)) return -2;
  return rd_ts_blocks(n * plane) * rd_ts_nsums(n_thresholds, max_lag) * (long)sizeof(double);       // (the scalar path has the most)
}

extern "C" int rdgan_temporal_accumulate(const float* x, long n, long day_stride, long plane, const double* thresholds,
                                         int n_thresholds, int max_lag, long long* counts_inout, double* sums_inout, void* workspace,
                                         long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!x || !counts_inout || !sums_inout || !workspace) return -2;
  if (!rd_aligned(7, counts_inout, sums_inout, workspace) || !rd_ts_shape_ok(n, plane, n_thresholds, max_lag)) return -2;
  if (!rd_hourly_layout_ok(x, n, day_stride, RD_HOURS * plane)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  if (workspace_bytes < rdgan_temporal_workspace_bytes(n, plane, n_thresholds, max_lag)) return -2;
  const bool vec = rd_vec4_ok(x, plane, day_stride);
  const int nblk = (int)rd_ts_blocks(vec ? n * (plane / 4) : n * plane), nsums = rd_ts_nsums(n_thresholds, max_lag);
  const size_t lds = rd_ts_lds_bytes(n_thresholds);
  hipStream_t st = (hipStream_t)stream;
#define RD_TS_LAUNCH(VV, KK)                                                                                                        \
  do {                                                                                                                              \
    RD_TRY(ensure_lds(nullptr, (const void*)k_temporal_accumulate<VV, KK>, rd_ts_lds_bytes(RD_TS_MAXT)));                           \
    hipLaunchKernelGGL((k_temporal_accumulate<VV, KK>), dim3((unsigned)nblk), dim3(RD_TS_THREADS), lds, st, x, n, day_stride, plane, \
                       thr, n_thresholds, max_lag, (unsigned long long*)counts_inout, (double*)workspace);                          \
  } while (0)
  if (vec && max_lag <= 6) RD_TS_LAUNCH(4, 6);
  else if (vec) RD_TS_LAUNCH(4, 12);
  else if (max_lag <= 6) RD_TS_LAUNCH(1, 6);
  else RD_TS_LAUNCH(1, 12);
#undef RD_TS_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_temporal_final, dim3((unsigned)nsums), dim3(RD_TS_THREADS), 0, st, (const double*)workspace, nblk, nsums,
                     sums_inout);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// rain cells of hourly fields (rdgan_cells.hip.h): connected wet areas, labelled and counted
// ------------------------------------------------------------------------------------
static bool rd_cl_shape_ok(long ny, long nx) {
  return ny >= 1 && nx >= 1 && ny <= RD_HOURLY_MAXPLANE && nx <= RD_HOURLY_MAXPLANE && ny * nx <= RD_HOURLY_MAXPLANE;
}

extern "C" long rdgan_cells_workspace_bytes(long ny, long nx, long planes_per_pass) {
  if (!rd_cl_shape_ok(ny, nx) || planes_per_pass < 1 || planes_per_pass > RD_CL_MAXPASS) return -2;
  return rd_cl_ws_bytes(ny * nx, planes_per_pass);
}

// The label front end cells and storms share: P planes from plane p0 on labelled tile by tile at one threshold, then the tiles
// merged along their borders.  The caller has raised k_cells_label_tile's LDS limit (ensure_lds, once per entry call, not here).
static void rd_cl_label_planes(hipStream_t st, const float* x, long day_stride, long ny, long nx, long p0, unsigned P, float thr,
                               int conn8, int first, unsigned long long* wet, unsigned long long* bad, unsigned long long* vol,
                               int* parent, unsigned* area, unsigned* words) {
  const int tiles_x = (int)((nx + RD_CL_TILE - 1) / RD_CL_TILE), tiles_y = (int)((ny + RD_CL_TILE - 1) / RD_CL_TILE);
  const long border = (long)(tiles_x - 1) * ny + (long)(tiles_y - 1) * nx;
  hipLaunchKernelGGL(k_cells_label_tile, dim3((unsigned)(tiles_x * tiles_y), P), dim3(RD_CL_THREADS), RD_CL_LDS_BYTES, st, x, day_stride,
                     (int)ny, (int)nx, p0, thr, conn8, first, wet, bad, vol, parent, area, words);
  if (border > 0)
    hipLaunchKernelGGL(k_cells_merge, dim3((unsigned)((border + RD_CL_THREADS - 1) / RD_CL_THREADS), P), dim3(RD_CL_THREADS), 0, st,
                       (int)ny, (int)nx, conn8, parent);
}

extern "C" int rdgan_cells_accumulate(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds,
                                      int n_thresholds, int connectivity, long long* counts_inout, int* labels_out,
                                      int label_threshold, void* workspace, long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!x || !counts_inout || !workspace) return -2;
  if (!rd_aligned(3, labels_out) || !rd_aligned(7, counts_inout, workspace)) return -2;
  if (!rd_cl_shape_ok(ny, nx) || (connectivity != 4 && connectivity != 8)) return -2;
  const long plane = ny * nx;
  if (!rd_hourly_layout_ok(x, n, day_stride, RD_HOURS * plane)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  if (labels_out && (label_threshold < 0 || label_threshold >= n_thresholds)) return -2;
  // the planes of a pass: as many as the workspace holds
  const long n_planes = n * RD_HOURS;
  const long per_pass = rd_pass_units(workspace_bytes, rd_cl_ws_bytes(plane, 1), n_planes, RD_CL_MAXPASS);
  if (per_pass < 1) return -2;
  unsigned long long* vol = (unsigned long long*)workspace;
  int* parent = (int*)(vol + per_pass * plane);
  unsigned* area = (unsigned*)(parent + per_pass * plane);
  unsigned* words = area + per_pass * plane;
  unsigned long long* counts = (unsigned long long*)counts_inout;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ensure_lds(nullptr, (const void*)k_cells_label_tile, RD_CL_LDS_BYTES));
  const int conn8 = connectivity == 8;
  for (long p0 = 0; p0 < n_planes; p0 += per_pass) {
    const unsigned P = (unsigned)std::min<long>(per_pass, n_planes - p0);
    for (int t = 0; t < n_thresholds; ++t) {
      unsigned long long* ct = counts + (long)t * RD_CL_NC;
      rd_cl_label_planes(st, x, day_stride, ny, nx, p0, P, thr.v[t], conn8, (int)(t == 0), ct + RD_CL_WET,
                         counts + (long)n_thresholds * RD_CL_NC + 1, vol, parent, area, words);
      hipLaunchKernelGGL(k_cells_resolve, dim3((unsigned)((plane + RD_CL_THREADS - 1) / RD_CL_THREADS), P), dim3(RD_CL_THREADS), 0, st, plane,
                         p0, vol, parent, area, labels_out && t == label_threshold ? labels_out : (int*)nullptr);
      hipLaunchKernelGGL(k_cells_reduce, dim3((unsigned)((plane + RD_CL_RCHUNK - 1) / RD_CL_RCHUNK), P), dim3(RD_CL_THREADS), 0, st, plane, p0,
                         (const unsigned long long*)vol, (const int*)parent, (const unsigned*)area, words, ct);
      hipLaunchKernelGGL(k_cells_planes, dim3((P + RD_CL_THREADS - 1) / RD_CL_THREADS), dim3(RD_CL_THREADS), 0, st, (int)P,
                         (const unsigned*)words, ct, t == 0 ? counts + (long)n_thresholds * RD_CL_NC : (unsigned long long*)nullptr);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// object-based verification (rdgan_sal.hip.h): the per-plane records of SAL on the cells' labels
// ------------------------------------------------------------------------------------
// the cells' limits, and every moment below 2^63: 2^21 max(ny, nx) ny nx < 2^63
static bool rd_sal_shape_ok(long ny, long nx) {
  return rd_cl_shape_ok(ny, nx) && (long long)std::max(ny, nx) * ny * nx < RD_SAL_MAXMOMENT;
}

extern "C" long rdgan_sal_workspace_bytes(long ny, long nx, long planes_per_pass) {
  if (!rd_sal_shape_ok(ny, nx) || planes_per_pass < 1 || planes_per_pass > RD_CL_MAXPASS) return -2;
  return rd_sal_ws_bytes(ny * nx, planes_per_pass);
}

extern "C" int rdgan_sal_records(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds, int n_thresholds,
                                 int connectivity, long long* plane_out, long long* obj_out, double* vr_out, void* workspace,
                                 long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!x || !plane_out || !obj_out || !vr_out || !workspace) return -2;
  if (!rd_aligned(7, plane_out, obj_out, vr_out, workspace)) return -2;
  if (!rd_sal_shape_ok(ny, nx) || (connectivity != 4 && connectivity != 8)) return -2;
  const long plane = ny * nx, day = RD_HOURS * plane;
  if (!rd_hourly_layout_ok((const void*)x, n, day_stride, day)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  // the planes of a pass: as many as the workspace holds
  const long n_planes = n * RD_HOURS, chunks = rd_sal_chunks(plane);
  const long per_pass = rd_pass_units(workspace_bytes, rd_sal_ws_bytes(plane, 1), n_planes, RD_CL_MAXPASS);
  if (per_pass < 1) return -2;
  unsigned long long* vol = (unsigned long long*)workspace;
  unsigned long long* obj = vol + per_pass * plane;
  unsigned long long* partial = obj + 4 * per_pass * plane;
  unsigned long long* sink = partial + RD_SAL_NPART * per_pass * chunks;   // wet counts by hour, read by nobody
  int* parent = (int*)(sink + RD_SAL_SINK * per_pass);
  unsigned* area = (unsigned*)(parent + per_pass * plane);
  unsigned* words = area + per_pass * plane;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ensure_lds(nullptr, (const void*)k_cells_label_tile, RD_CL_LDS_BYTES));
  hipError_t e = hipMemsetAsync(plane_out, 0, (size_t)n_planes * 4 * sizeof(long long), st);       // the whole-plane sums are added
  if (e != hipSuccess) return (int)e;
  const int conn8 = connectivity == 8;
  const unsigned pblocks = (unsigned)((plane + RD_SAL_THREADS - 1) / RD_SAL_THREADS);
  for (long p0 = 0; p0 < n_planes; p0 += per_pass) {
    const unsigned P = (unsigned)std::min<long>(per_pass, n_planes - p0);
    for (int t = 0; t < n_thresholds; ++t) {
      rd_cl_label_planes(st, x, day_stride, ny, nx, p0, P, thr.v[t], conn8, 0, sink, sink, vol, parent, area, words);
      hipLaunchKernelGGL(k_cells_resolve, dim3((unsigned)((plane + RD_CL_THREADS - 1) / RD_CL_THREADS), P), dim3(RD_CL_THREADS), 0, st, plane,
                         p0, vol, parent, area, (int*)nullptr);
      hipLaunchKernelGGL(k_sal_clear, dim3(pblocks, P), dim3(RD_SAL_THREADS), 0, st, plane, (const int*)parent, obj);
      hipLaunchKernelGGL(k_sal_moments, dim3(pblocks, P), dim3(RD_SAL_THREADS), 0, st, x, day_stride, (int)nx, plane, p0, (int)(t == 0),
                         (const int*)parent, obj, (unsigned long long*)plane_out);
      hipLaunchKernelGGL(k_sal_plane, dim3((unsigned)chunks, P), dim3(RD_SAL_THREADS), 0, st, plane, p0, (const int*)parent,
                         (const unsigned*)area, (const unsigned long long*)obj, (const unsigned long long*)plane_out, partial);
      hipLaunchKernelGGL(k_sal_final, dim3(P), dim3(64), 0, st, chunks, p0, t, n_thresholds, (const unsigned long long*)partial, obj_out,
                         vr_out);
      e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// scale-separation verification (rdgan_iss.hip.h): the integer state of the intensity-scale skill score
// ------------------------------------------------------------------------------------
static bool rd_iss_shape_ok(long ny, long nx, int levels) {
  return rd_cl_shape_ok(ny, nx) && levels >= 1 && levels <= RD_ISS_MAXL && (1L << levels) <= std::min(ny, nx);
}

extern "C" long rdgan_iss_workspace_bytes(long ny, long nx, int levels, long pairs_per_pass) {
  if (!rd_iss_shape_ok(ny, nx, levels) || pairs_per_pass < 1 || pairs_per_pass > (1L << 30)) return -2;
  return pairs_per_pass * rd_iss_pair_bytes(ny, nx, levels);
}

// member slices of a launch of k_iss_tiles: enough workgroups to fill the device, at least 8 members each where there are as many
static unsigned rd_iss_split(long workgroups, int nm) {
  const long want = (2048 + workgroups - 1) / workgroups, most = (nm + 7) / 8;
  return (unsigned)std::max<long>(1, std::min<long>(std::min<long>(want, most), RD_ISS_MAXSPLIT));
}

extern "C" int rdgan_iss_accumulate(const float* members, int s, long member_stride, const float* obs, long n_days, long ny, long nx,
                                    const double* thresholds, int n_thresholds, int levels, long long* counts_inout,
                                    long long* tiles_inout, void* workspace, long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!members || !obs || !counts_inout || !tiles_inout || !workspace) return -2;
  if (!rd_aligned(3, members, obs) || !rd_aligned(7, counts_inout, tiles_inout, workspace)) return -2;
  if (s < 1 || s > RD_ISS_MAXS || n_days < 1 || !rd_iss_shape_ok(ny, nx, levels)) return -2;
  const long plane = ny * nx;
  if (n_days > RD_HOURLY_MAXELEMS / (RD_HOURS * plane)) return -2;
  const long P = n_days * RD_HOURS * plane;
  if (!rd_hourly_layout_ok((const void*)members, (long)s, member_stride, P)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  const rd_iss_geo g = rd_iss_geometry(ny, nx, levels);
  const long units = (n_days + g.G - 1) / g.G * RD_HOURS, nblocks = (long)g.nby * g.nbx;
  const long per_pass = rd_pass_units(workspace_bytes, rd_iss_pair_bytes(ny, nx, levels), (long)s * units, 1L << 30);
  if (per_pass < 1) return -2;
  const int T = n_thresholds;
  unsigned long long* counts = (unsigned long long*)counts_inout;
  unsigned long long* tiles = (unsigned long long*)tiles_inout;
  hipStream_t st = (hipStream_t)stream;
  if (levels <= 6) {                       // nothing is held back: every member in one launch per RD_ISS_MAXUNITS units
    for (long u0 = 0; u0 < units; u0 += RD_ISS_MAXUNITS) {
      const unsigned nu = (unsigned)std::min<long>(RD_ISS_MAXUNITS, units - u0);
      hipLaunchKernelGGL(k_iss_tiles, dim3((unsigned)nblocks, nu, rd_iss_split(nblocks * nu, s)), dim3(RD_ISS_THREADS), 0, st, members,
                         member_stride, 0, s, obs, n_days, g, thr, T, u0, counts, tiles, (unsigned*)nullptr, (unsigned*)nullptr);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
  // the pairs of a pass: every member of as many units as the workspace holds, or of one unit as many members as it holds
  const int nm = (int)std::min<long>(per_pass, s);
  const long nu_pass = per_pass >= s ? std::min<long>(std::min<long>(per_pass / s, units), RD_ISS_MAXUNITS) : 1;
  unsigned* held = (unsigned*)workspace;
  unsigned* flags = held + (long)nm * nu_pass * nblocks * T * 4 * RD_ISS_REC;
  const unsigned n_tiles = (unsigned)((g.cy >> levels) * (g.cx >> levels));
  for (long u0 = 0; u0 < units; u0 += nu_pass) {
    const unsigned nu = (unsigned)std::min<long>(nu_pass, units - u0);
    for (int m0 = 0; m0 < s; m0 += nm) {
      const int n = std::min(nm, s - m0);
      hipLaunchKernelGGL(k_iss_tiles, dim3((unsigned)nblocks, nu, rd_iss_split(nblocks * nu, n)), dim3(RD_ISS_THREADS), 0, st, members,
                         member_stride, m0, n, obs, n_days, g, thr, T, u0, counts, tiles, held, flags);
      hipLaunchKernelGGL(k_iss_upper, dim3(n_tiles, nu, (unsigned)n), dim3(RD_ISS_THREADS), 0, st, (const unsigned*)held,
                         (const unsigned*)flags, g, T, u0, counts, tiles);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// distance-map verification (rdgan_distmap.hip.h): exact distance transforms of event sets and the records of pairs
// ------------------------------------------------------------------------------------
static bool rd_dm_shape_ok(long ny, long nx) { return ny >= 1 && nx >= 1 && ny <= RD_DM_MAXSIDE && nx <= RD_DM_MAXSIDE; }

extern "C" long rdgan_dm_workspace_bytes(long ny, long nx, long planes_per_pass) {
  if (!rd_dm_shape_ok(ny, nx) || planes_per_pass < 1 || planes_per_pass > RD_DM_MAXPASS) return -2;
  return planes_per_pass * rd_dm_plane_bytes(ny, nx);
}

// One pass: pack P planes from plane q0 on and transform them.  maps_out: the maps of the planes (records null), or records: the
// records of the planes against obs / obs_maps.  sizes: P * T words, zeroed here unless they are the caller's output
static int rd_dm_pass(hipStream_t st, const rd_dm_geo& g, const float* x, long outer_stride, long per_outer, long q0, long P,
                      const rd_thr& thr, int T, unsigned long long* masks, unsigned long long* sizes, bool zero_sizes,
                      unsigned short* maps_out, const float* obs, const unsigned short* obs_maps, int cutoff, unsigned long long* records) {
  if (zero_sizes) {
    hipError_t e = hipMemsetAsync(sizes, 0, (size_t)P * T * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
  }
  const long items = (long)g.ny * g.W, chunk = 4 * RD_DM_PACK_ITEMS;
  hipLaunchKernelGGL(k_dm_pack, dim3((unsigned)P, (unsigned)((items + chunk - 1) / chunk)), dim3(RD_DM_THREADS), 0, st, x, outer_stride,
                     per_outer, q0, g.ny, g.nx, g.W, thr, T, masks, sizes);
  const dim3 grid((unsigned)((P + g.G - 1) / g.G * g.nstrips), (unsigned)T);
  if (records)
    hipLaunchKernelGGL(k_dm_transform<true>, grid, dim3(RD_DM_THREADS), rd_dm_lds_bytes(g), st, g, q0, (int)P, T,
                       (const unsigned long long*)masks, (const unsigned long long*)sizes, (unsigned short*)nullptr, obs, obs_maps,
                       per_outer, thr, cutoff, records);
  else
    hipLaunchKernelGGL(k_dm_transform<false>, grid, dim3(RD_DM_THREADS), rd_dm_lds_bytes(g), st, g, q0, (int)P, T,
                       (const unsigned long long*)masks, (const unsigned long long*)sizes, maps_out, (const float*)nullptr,
                       (const unsigned short*)nullptr, per_outer, thr, 0, (unsigned long long*)nullptr);
  return (int)hipGetLastError();
}

extern "C" int rdgan_dm_maps(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds, int n_thresholds,
                             unsigned short* maps_out, long long* set_sizes_out, void* workspace, long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!x || !maps_out || !set_sizes_out || !workspace) return -2;
  if (!rd_aligned(1, maps_out) || !rd_aligned(7, set_sizes_out, workspace) || !rd_dm_shape_ok(ny, nx)) return -2;
  const long plane = ny * nx;
  if (!rd_hourly_layout_ok((const void*)x, n, day_stride, RD_HOURS * plane)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  const long n_planes = n * RD_HOURS;
  const long per_pass = rd_pass_units(workspace_bytes, rd_dm_plane_bytes(ny, nx), n_planes, RD_DM_MAXPASS);
  if (per_pass < 1) return -2;
  const rd_dm_geo g = rd_dm_geometry(ny, nx);
  const int T = n_thresholds;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ensure_lds(nullptr, (const void*)k_dm_transform<false>, rd_dm_lds_bytes(g)));
  hipError_t e = hipMemsetAsync(set_sizes_out, 0, (size_t)n_planes * T * sizeof(long long), st);       // the set sizes are added
  if (e != hipSuccess) return (int)e;
  for (long q0 = 0; q0 < n_planes; q0 += per_pass) {
    const long P = std::min<long>(per_pass, n_planes - q0);
    RD_TRY(rd_dm_pass(st, g, x, day_stride, RD_HOURS, q0, P, thr, T, (unsigned long long*)workspace,
                      (unsigned long long*)set_sizes_out + q0 * T, false, maps_out, nullptr, nullptr, 0, nullptr));
  }
  return 0;
}

extern "C" int rdgan_dm_records(const float* members, int s, long member_stride, const float* obs, const unsigned short* obs_maps,
                                long n_days, long ny, long nx, const double* thresholds, int n_thresholds, int cutoff16,
                                long long* records_out, void* workspace, long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!members || !obs || !obs_maps || !records_out || !workspace) return -2;
  if (!rd_aligned(3, members, obs) || !rd_aligned(1, obs_maps) || !rd_aligned(7, records_out, workspace)) return -2;
  if (s < 1 || s > RD_DM_MAXS || n_days < 1 || !rd_dm_shape_ok(ny, nx) || cutoff16 < RD_DM_CMIN || cutoff16 > RD_DM_CMAX) return -2;
  const long plane = ny * nx;
  if (n_days > RD_HOURLY_MAXELEMS / (RD_HOURS * plane)) return -2;
  const long per_member = n_days * RD_HOURS;
  if (!rd_hourly_layout_ok((const void*)members, (long)s, member_stride, per_member * plane)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  const long n_planes = (long)s * per_member;
  const long per_pass = rd_pass_units(workspace_bytes, rd_dm_plane_bytes(ny, nx), n_planes, RD_DM_MAXPASS);
  if (per_pass < 1) return -2;
  const rd_dm_geo g = rd_dm_geometry(ny, nx);
  const int T = n_thresholds;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ensure_lds(nullptr, (const void*)k_dm_transform<true>, rd_dm_lds_bytes(g)));
  hipError_t e = hipMemsetAsync(records_out, 0, (size_t)n_planes * T * RD_DM_NREC * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  unsigned long long* masks = (unsigned long long*)workspace;
  unsigned long long* sizes = masks + per_pass * (1 + RD_THR_MAX) * ny * g.W;
  for (long q0 = 0; q0 < n_planes; q0 += per_pass) {
    const long P = std::min<long>(per_pass, n_planes - q0);
    RD_TRY(rd_dm_pass(st, g, members, member_stride, per_member, q0, P, thr, T, masks, sizes, true, nullptr, obs, obs_maps, cutoff16,
                      (unsigned long long*)records_out));
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// storms of hourly fields (rdgan_storms.hip.h): wet volumes connected through the day's hours, labelled and counted
// ------------------------------------------------------------------------------------
static bool rd_sm_shape_ok(long ny, long nx) { return rd_cl_shape_ok(ny, nx) && RD_HOURS * ny * nx <= RD_SM_MAXDAY; }

extern "C" long rdgan_storms_state_count(int n_thresholds) {
  if (n_thresholds < 1 || n_thresholds > RD_CL_MAXT) return -2;
  return (long)n_thresholds * RD_SM_NC + 2;
}

extern "C" long rdgan_storms_workspace_bytes(long ny, long nx, long days_per_pass) {
  if (!rd_sm_shape_ok(ny, nx) || days_per_pass < 1 || days_per_pass > RD_SM_MAXPASS) return -2;
  return rd_sm_ws_bytes(ny * nx, days_per_pass);
}

extern "C" int rdgan_storms_accumulate(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds,
                                       int n_thresholds, int connectivity, int reach, long long* counts_inout, int* labels_out,
                                       int label_threshold, void* workspace, long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!x || !counts_inout || !workspace) return -2;
  if (!rd_aligned(3, labels_out) || !rd_aligned(7, counts_inout, workspace)) return -2;
  if (!rd_sm_shape_ok(ny, nx) || (connectivity != 4 && connectivity != 8) || reach < 0 || reach > RD_SM_MAXREACH) return -2;
  const long plane = ny * nx, V = RD_HOURS * plane;
  if (!rd_hourly_layout_ok(x, n, day_stride, V)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr)) return -2;
  if (labels_out && (label_threshold < 0 || label_threshold >= n_thresholds)) return -2;
  // the days of a pass: as many whole days as the workspace holds
  const long per_pass = rd_pass_units(workspace_bytes, rd_sm_ws_bytes(plane, 1), n, RD_SM_MAXPASS);
  if (per_pass < 1) return -2;
  unsigned long long* vol = (unsigned long long*)workspace;
  int* parent = (int*)(vol + per_pass * V);
  unsigned* area = (unsigned*)(parent + per_pass * V);
  unsigned* last = area + per_pass * V;
  unsigned* day_words = last + 2 * per_pass * V;                          // (behind the spare word of every voxel)
  unsigned* plane_words = day_words + 2 * per_pass;
  unsigned long long* counts = (unsigned long long*)counts_inout;
  unsigned long long* tail = counts + (long)n_thresholds * RD_SM_NC;      // n_days, n_bad_pixels
  hipStream_t st = (hipStream_t)stream;
  RD_TRY(ensure_lds(nullptr, (const void*)k_cells_label_tile, RD_CL_LDS_BYTES));
  const int conn8 = connectivity == 8;
  const unsigned vblocks = (unsigned)((V + RD_CL_THREADS - 1) / RD_CL_THREADS);
  for (long d0 = 0; d0 < n; d0 += per_pass) {
    const unsigned D = (unsigned)std::min<long>(per_pass, n - d0), P = D * RD_HOURS;
    for (int t = 0; t < n_thresholds; ++t) {
      unsigned long long* ct = counts + (long)t * RD_SM_NC;
      rd_cl_label_planes(st, x, day_stride, ny, nx, d0 * RD_HOURS, P, thr.v[t], conn8, (int)(t == 0), ct + RD_SM_WET, tail + 1, vol,
                         parent, area, plane_words);
      hipLaunchKernelGGL(k_storm_lift, dim3(vblocks, D), dim3(RD_CL_THREADS), 0, st, plane, parent, last, day_words);
      hipLaunchKernelGGL(k_storm_link, dim3((unsigned)((V - plane + RD_CL_THREADS - 1) / RD_CL_THREADS), D), dim3(RD_CL_THREADS), 0, st, (int)ny,
                         (int)nx, reach, parent);
      hipLaunchKernelGGL(k_storm_resolve, dim3(vblocks, D), dim3(RD_CL_THREADS), 0, st, plane, d0, vol, parent, area, last,
                         labels_out && t == label_threshold ? labels_out : (int*)nullptr);
      hipLaunchKernelGGL(k_storm_reduce, dim3((unsigned)((V + RD_SM_RCHUNK - 1) / RD_SM_RCHUNK), D), dim3(RD_CL_THREADS), 0, st, plane,
                         (const unsigned long long*)vol, (const int*)parent, (const unsigned*)area, (const unsigned*)last, day_words, ct);
      hipLaunchKernelGGL(k_storm_days, dim3((D + RD_CL_THREADS - 1) / RD_CL_THREADS), dim3(RD_CL_THREADS), 0, st, (int)D,
                         (const unsigned*)day_words, ct, t == 0 ? tail : (unsigned long long*)nullptr);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// areal extremes of hourly fields (rdgan_areal.hip.h): the largest k-hour accumulation over any w x w box, per day
// ------------------------------------------------------------------------------------
// a strictly increasing list of 1 .. n_max whole numbers in lo .. hi
static bool rd_increasing(const int* v, int n, int n_max, int lo, int hi) {
  if (!v || n < 1 || n > n_max) return false;
  for (int i = 0; i < n; ++i)
    if (v[i] < lo || v[i] > hi || (i > 0 && v[i] <= v[i - 1])) return false;
  return true;
}

// the three lists as the kernels take them; false for a list out of range.  The internal widths are 1 and then the caller's others.
static bool rd_ar_make_lists(const int* windows, int K, const int* widths, int W, const double* levels, int L, long max_width,
                             rd_ar_lists* out) {
  if (!rd_increasing(windows, K, RD_AR_MAXK, 1, RD_HOURS) || !rd_increasing(widths, W, RD_AR_MAXW, 1, RD_AR_MAXWIDTH)) return false;
  if (widths[W - 1] > max_width) return false;
  rd_ar_lists a = {};
  a.K = K, a.W = W, a.L = L, a.slots = 1;
  a.slot_width[0] = 1;
  for (int i = 0; i < K; ++i) a.windows[i] = windows[i];
  for (int i = 0; i < W; ++i) {
    a.widths[i] = widths[i];
    a.slot_of[i] = widths[i] == 1 ? 0 : a.slots;
    if (widths[i] != 1) a.slot_width[a.slots++] = widths[i];
  }
  if (!rd_levels_q(levels, L, RD_AR_MAXL, a.level_q)) return false;
  *out = a;
  return true;
}

static bool rd_ar_shape_ok(long ny, long nx) {
  return ny >= 1 && nx >= 1 && ny <= RD_HOURLY_MAXPLANE && nx <= RD_HOURLY_MAXPLANE && ny * nx <= RD_HOURLY_MAXPLANE;
}

extern "C" long rdgan_areal_state_count(int n_windows, int n_widths, int n_levels) {
  if (n_windows < 1 || n_windows > RD_AR_MAXK || n_widths < 1 || n_widths > RD_AR_MAXW || n_levels < 0 || n_levels > RD_AR_MAXL) return -2;
  return rd_ar_state_count(n_windows, n_widths, n_levels);
}

extern "C" long rdgan_areal_workspace_bytes(long ny, long nx, long days_per_pass) {
  if (!rd_ar_shape_ok(ny, nx) || days_per_pass < 1 || days_per_pass > RD_AR_MAXPASS) return -2;
  return days_per_pass * rd_ar_day_bytes(ny * nx);
}

extern "C" int rdgan_areal_accumulate(const float* x, long n, long day_stride, long ny, long nx, const int* windows, int n_windows,
                                      const int* widths, int n_widths, const double* levels, int n_levels, long long* counts_inout,
                                      long long* depths_out, void* workspace, long workspace_bytes, void* stream) {
  rd_ar_lists lists;
  if (!x || !counts_inout || !workspace) return -2;
  if (!rd_aligned(7, counts_inout, depths_out, workspace) || !rd_ar_shape_ok(ny, nx)) return -2;
  const long plane = ny * nx, V = RD_HOURS * plane;
  if (!rd_hourly_layout_ok(x, n, day_stride, V)) return -2;
  if (!rd_ar_make_lists(windows, n_windows, widths, n_widths, levels, n_levels, std::min(ny, nx), &lists)) return -2;
  // the days of a pass: as many whole days as the workspace holds
  const long per_pass = rd_pass_units(workspace_bytes, rd_ar_day_bytes(plane), n, RD_AR_MAXPASS);
  if (per_pass < 1) return -2;
  unsigned long long* keys = (unsigned long long*)workspace;
  int* S = (int*)(keys + per_pass * RD_AR_DAY_KEYS);
  unsigned char* B = (unsigned char*)(S + per_pass * V);
  unsigned long long* counts = (unsigned long long*)counts_inout;
  unsigned long long* tail = counts + rd_ar_state_count(lists.K, lists.W, lists.L) - 2;   // n_days_total, n_bad
  hipStream_t st = (hipStream_t)stream;
  const int wmax = lists.slot_width[lists.slots - 1];
  const size_t lds = rd_ar_lds_bytes(wmax);
  RD_TRY(ensure_lds(nullptr, (const void*)k_areal_boxes, rd_ar_lds_bytes(RD_AR_MAXWIDTH)));
  const bool vec = rd_vec4_ok(x, plane, day_stride) && rd_aligned(15, S);
  const int tiles_x = (int)((nx + RD_AR_TILE - 1) / RD_AR_TILE), tiles_y = (int)((ny + RD_AR_TILE - 1) / RD_AR_TILE);
  for (long d0 = 0; d0 < n; d0 += per_pass) {
    const unsigned D = (unsigned)std::min<long>(per_pass, n - d0);
    if (vec)
      hipLaunchKernelGGL(k_areal_prefix<4>, dim3((unsigned)((plane / 4 + RD_AR_THREADS - 1) / RD_AR_THREADS), D), dim3(RD_AR_THREADS), 0, st, x,
                         day_stride, plane, d0, keys, S, B, tail + 1);
    else
      hipLaunchKernelGGL(k_areal_prefix<1>, dim3((unsigned)((plane + RD_AR_THREADS - 1) / RD_AR_THREADS), D), dim3(RD_AR_THREADS), 0, st, x,
                         day_stride, plane, d0, keys, S, B, tail + 1);
    hipLaunchKernelGGL(k_areal_boxes, dim3((unsigned)(tiles_x * tiles_y), (unsigned)lists.K, D), dim3(RD_AR_THREADS), lds, st, (int)ny, (int)nx,
                       tiles_x, lists, wmax, (const int*)S, (const unsigned char*)B, keys);
    hipLaunchKernelGGL(k_areal_days, dim3((D + RD_AR_THREADS - 1) / RD_AR_THREADS, (unsigned)(lists.K * lists.W)), dim3(RD_AR_THREADS), 0, st,
                       (int)D, d0, lists, (const unsigned long long*)keys, counts, depths_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// catchment rainfall of hourly fields (rdgan_catchment.hip.h): hyetographs and k-hour maxima per basin of a map, per day
// ------------------------------------------------------------------------------------
static bool rd_ct_make_lists(const int* windows, int K, const double* levels, int L, rd_ct_lists* out) {
  if (!rd_increasing(windows, K, RD_CT_MAXK, 1, RD_HOURS)) return false;
  rd_ct_lists a = {};
  a.K = K, a.L = L;
  for (int i = 0; i < K; ++i) a.windows[i] = windows[i];
  if (!rd_levels_q(levels, L, RD_CT_MAXL, a.level_q)) return false;
  *out = a;
  return true;
}

extern "C" long rdgan_catchment_state_count(int n_catch, int n_windows, int n_levels) {
  if (n_catch < 1 || n_catch > RD_CT_MAXCATCH || n_windows < 1 || n_windows > RD_CT_MAXK || n_levels < 0 || n_levels > RD_CT_MAXL) return -2;
  return rd_ct_state_count(n_catch, n_windows, n_levels);
}

extern "C" long rdgan_catchment_workspace_bytes(int n_catch, long days_per_pass) {
  if (n_catch < 1 || n_catch > RD_CT_MAXCATCH || days_per_pass < 1 || days_per_pass > RD_CT_MAXPASS) return -2;
  return days_per_pass * rd_ct_day_bytes(n_catch);
}

extern "C" int rdgan_catchment_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, const int* chunks, long n_chunks,
                                          const int* pixels, long n_entries, const int* npix, int n_catch, const int* windows,
                                          int n_windows, const double* levels, int n_levels, long long* counts_inout,
                                          long long* series_out, long long* depths_out, void* workspace, long workspace_bytes,
                                          void* stream) {
  rd_ct_lists lists;
  if (!hourly || !chunks || !pixels || !npix || !counts_inout || !workspace) return -2;
  if (!rd_aligned(3, chunks, pixels, npix) || !rd_aligned(7, counts_inout, series_out, depths_out, workspace)) return -2;
  if (!rd_ar_shape_ok(ny, nx) || n_catch < 1 || n_catch > RD_CT_MAXCATCH) return -2;
  if (n_entries < n_catch || n_entries > RD_CT_MAXENTRIES || n_chunks < n_catch || n_chunks > n_entries || n_chunks > RD_CT_MAXCHUNKS) return -2;
  const long plane = ny * nx;
  if (!rd_hourly_layout_ok(hourly, n, day_stride, RD_HOURS * plane)) return -2;
  if (!rd_ct_make_lists(windows, n_windows, levels, n_levels, &lists)) return -2;
  // the days of a pass: as many whole days as the workspace holds and one launch has workgroups for
  const long per_pass = rd_pass_units(workspace_bytes, rd_ct_day_bytes(n_catch), n, std::min<long>(RD_CT_MAXPASS, RD_CT_MAXGROUPS / n_chunks));
  if (per_pass < 1) return -2;
  unsigned long long* P = (unsigned long long*)workspace;
  unsigned* B = (unsigned*)(P + per_pass * n_catch * RD_HOURS);
  hipStream_t st = (hipStream_t)stream;
  for (long d0 = 0; d0 < n; d0 += per_pass) {
    const long D = std::min<long>(per_pass, n - d0);
    RD_TRY((int)hipMemsetAsync(workspace, 0, (size_t)(per_pass * rd_ct_day_bytes(n_catch)), st));     // P and B of the pass
    hipLaunchKernelGGL(k_catch_sums, dim3((unsigned)n_chunks, (unsigned)D), dim3(RD_CT_THREADS), 0, st, hourly, day_stride, plane, d0, chunks,
                       pixels, n_entries, n_catch, P, B);
    hipLaunchKernelGGL(k_catch_days, dim3((unsigned)((D * n_catch + RD_CT_THREADS - 1) / RD_CT_THREADS)), dim3(RD_CT_THREADS), 0, st, (int)D, d0,
                       n_catch, lists, npix, (const unsigned long long*)P, (const unsigned*)B, (unsigned long long*)counts_inout, series_out,
                       depths_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// scaling of hourly fields (rdgan_scaling.hip.h): moments and histograms of box sums over dyadic boxes and aligned windows
// ------------------------------------------------------------------------------------
static bool rd_sc_args_ok(long ny, long nx, int space_levels) {
  return rd_ar_shape_ok(ny, nx) && space_levels >= 0 && space_levels <= RD_SC_MAXA && (1L << space_levels) <= std::min(ny, nx);
}

extern "C" long rdgan_scaling_state_count(int space_levels) {
  if (space_levels < 0 || space_levels > RD_SC_MAXA) return -2;
  return rd_sc_state_count(space_levels);
}

extern "C" long rdgan_scaling_workspace_bytes(long ny, long nx, int space_levels) {
  return rd_sc_args_ok(ny, nx, space_levels) ? RD_SC_WORKSPACE : -2;
}

extern "C" int rdgan_scaling_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, int space_levels,
                                        long long* counts_inout, void* workspace, long workspace_bytes, void* stream) {
  if (!hourly || !counts_inout || !workspace || !rd_aligned(7, counts_inout, workspace)) return -2;
  if (!rd_sc_args_ok(ny, nx, space_levels) || workspace_bytes < RD_SC_WORKSPACE) return -2;
  if (!rd_hourly_layout_ok(hourly, n, day_stride, RD_HOURS * ny * nx)) return -2;
  const rd_sc_geo g = rd_sc_geometry(ny, nx, space_levels);
  const long units = (n + g.G - 1) / g.G * g.nby * g.nbx;
  // a side of 64 or more fills more than half of its blocks' side, a shorter one more than half of its share: the units of a call
  // hold fewer than 4 pixels for each of the array's (the last collage apart), a workgroup's share stays below RD_SC_MAXUNITS
  static_assert(4 * (RD_HOURLY_MAXELEMS / (RD_HOURS * RD_SC_TILE * RD_SC_TILE)) / RD_SC_MINGRID + 2 <= RD_SC_MAXUNITS, "32-bit LDS counters");
  const unsigned blocks = (unsigned)std::min<long>(units, RD_SC_MINGRID);
  if (rd_vec4_ok(hourly, nx, day_stride))
    hipLaunchKernelGGL(k_scaling_tiles<4>, dim3(blocks), dim3(RD_SC_THREADS), 0, (hipStream_t)stream, hourly, n, day_stride, g, units,
                       (unsigned long long*)counts_inout);
  else
    hipLaunchKernelGGL(k_scaling_tiles<1>, dim3(blocks), dim3(RD_SC_THREADS), 0, (hipStream_t)stream, hourly, n, day_stride, g, units,
                       (unsigned long long*)counts_inout);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// space-time structure of hourly fields (rdgan_spacetime.hip.h): displaced wet/dry agreement and the best shift of hour pairs
// ------------------------------------------------------------------------------------
static bool rd_st_params_ok(int n_thresholds, int radius, int max_lag) {
  return n_thresholds >= 1 && n_thresholds <= RD_ST_MAXT && radius >= 1 && radius <= RD_ST_MAXR && max_lag >= 1 && max_lag <= RD_ST_MAXK;
}

static bool rd_st_shape_ok(long ny, long nx, long least) {
  return ny >= least && nx >= least && ny <= RD_HOURLY_MAXPLANE && nx <= RD_HOURLY_MAXPLANE && ny * nx <= RD_HOURLY_MAXPLANE;
}

extern "C" long rdgan_spacetime_state_count(int n_thresholds, int radius, int max_lag) {
  if (!rd_st_params_ok(n_thresholds, radius, max_lag)) return -2;
  return rd_st_state_count(n_thresholds, radius, max_lag);
}

extern "C" long rdgan_spacetime_workspace_bytes(long ny, long nx, int n_thresholds, long planes_per_pass) {
  if (!rd_st_shape_ok(ny, nx, 1) || n_thresholds < 1 || n_thresholds > RD_ST_MAXT || planes_per_pass < 1 || planes_per_pass > RD_ST_MAXPASS)
    return -2;
  return planes_per_pass * rd_st_plane_bytes(ny, nx, n_thresholds);
}

extern "C" int rdgan_spacetime_accumulate(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds,
                                          int n_thresholds, int radius, int max_lag, long long* counts_inout, void* workspace,
                                          long workspace_bytes, void* stream) {
  rd_thr thr;
  if (!x || !counts_inout || !workspace) return -2;
  if (!rd_aligned(7, counts_inout, workspace)) return -2;
  if (!rd_thresholds(thresholds, n_thresholds, &thr) || !rd_st_params_ok(n_thresholds, radius, max_lag)) return -2;
  if (!rd_st_shape_ok(ny, nx, 2 * radius + 1)) return -2;
  if (!rd_hourly_layout_ok(x, n, day_stride, RD_HOURS * ny * nx)) return -2;
  // the days of a pass: as many whole days as the workspace holds
  const long per_pass = rd_pass_units(workspace_bytes, RD_HOURS * rd_st_plane_bytes(ny, nx, n_thresholds), n, RD_ST_MAXPASS / RD_HOURS);
  if (per_pass < 1) return -2;
  const int W = (int)((nx + 63) / 64), T = n_thresholds;
  int cw, bh;
  rd_st_tile(ny, nx, radius, &cw, &bh);
  const int ns = rd_st_slices(radius, bh);
  const size_t lds = rd_st_lds_bytes(radius, cw, bh);
  const bool vec = rd_vec4_ok(x, nx, day_stride);
  unsigned long long* counts = (unsigned long long*)counts_inout;
  unsigned long long* tail = counts + rd_st_thr_base(radius, max_lag, T);                 // n_days, n_bad_pixels
  unsigned long long* masks = (unsigned long long*)workspace;
  hipStream_t st = (hipStream_t)stream;
  for (long d0 = 0; d0 < n; d0 += per_pass) {
    const long days = std::min<long>(per_pass, n - d0);
    const long waves = days * RD_HOURS * ny * (vec ? (W + 3) / 4 : W);
    const unsigned blocks = (unsigned)std::min<long>((waves + RD_ST_THREADS / 64 - 1) / (RD_ST_THREADS / 64), RD_ST_PACK_MAXBLOCKS);
    if (vec)
      hipLaunchKernelGGL(k_st_pack<4>, dim3(blocks), dim3(RD_ST_THREADS), 0, st, x, day_stride, (int)ny, (int)nx, W, d0, days, thr, T, masks,
                         tail, tail + 1);
    else
      hipLaunchKernelGGL(k_st_pack<1>, dim3(blocks), dim3(RD_ST_THREADS), 0, st, x, day_stride, (int)ny, (int)nx, W, d0, days, thr, T, masks,
                         tail, tail + 1);
    hipLaunchKernelGGL(k_st_correlate, dim3((unsigned)(days * (max_lag + 1) * RD_ST_GROUPS), (unsigned)T), dim3(RD_ST_THREADS), lds, st,
                       (const unsigned long long*)masks, (int)ny, (int)nx, W, T, radius, max_lag, cw, bh, ns, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// analog baseline (rdgan_analog.hip.h): the nearest library days of a daily condition and their scaled hourly fractions
// ------------------------------------------------------------------------------------
static bool rd_an_shape_ok(long ny, long nx) { return ny >= 1 && nx >= 1 && ny <= RD_AN_MAXP && nx <= RD_AN_MAXP && ny * nx <= RD_AN_MAXP; }

extern "C" long rdgan_analog_workspace_bytes(long n_queries, int k, long n_slices) {
  if (n_queries < 1 || n_queries > RD_AN_MAXQ || k < 1 || k > RD_AN_MAXK || n_slices < 1 || n_slices > rd_an_blocks(RD_AN_MAXN)) return -2;
  return n_slices * rd_an_list_bytes(n_queries, k);
}

extern "C" int rdgan_analog_features(const float* x, long n, long day_stride, long ny, long nx, int hourly, unsigned short* feat_out,
                                     unsigned short* mask_out, long long* total_out, unsigned char* void_out, long long* n_void_out,
                                     void* stream) {
  if (!x || !feat_out || ((unsigned long long)x & 3) || ((unsigned long long)feat_out & 15)) return -2;
  if (n < 1 || !rd_an_shape_ok(ny, nx)) return -2;
  const long plane = ny * nx, ppad = rd_an_ppad(plane);
  const int C = (int)(ppad / 8);
  hipStream_t st = (hipStream_t)stream;
  if (!hourly) {                                                           // the conditions of the queries, [n][plane]
    if (!mask_out || ((unsigned long long)mask_out & 15) || total_out || void_out || n_void_out) return -2;
    if (n > RD_AN_MAXQ || day_stride != plane) return -2;
    hipLaunchKernelGGL(k_analog_query, dim3((unsigned)((n * ppad + 255) / 256)), dim3(256), 0, st, x, n, (int)plane, (int)ppad, feat_out, mask_out);
    return (int)hipGetLastError();
  }
  if (mask_out || !total_out || !void_out || !n_void_out || (((unsigned long long)total_out | (unsigned long long)n_void_out) & 7)) return -2;
  if (n > RD_AN_MAXN || !rd_day_stride_ok(n, day_stride, RD_HOURS * plane)) return -2;
  RD_TRY((int)hipMemsetAsync(total_out, 0, (size_t)n * 8, st));
  RD_TRY((int)hipMemsetAsync(n_void_out, 0, 8, st));
  const unsigned blocks = (unsigned)((n * C + 255) / 256);
  if (rd_vec4_ok(x, plane, day_stride))
    hipLaunchKernelGGL(k_analog_features<true>, dim3(blocks), dim3(256), 0, st, x, n, day_stride, (int)plane, C, (uint4*)feat_out,
                       (unsigned long long*)total_out);
  else
    hipLaunchKernelGGL(k_analog_features<false>, dim3(blocks), dim3(256), 0, st, x, n, day_stride, (int)plane, C, (uint4*)feat_out,
                       (unsigned long long*)total_out);
  hipLaunchKernelGGL(k_analog_days, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (unsigned long long*)total_out, void_out,
                     (unsigned long long*)n_void_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_analog_search(const unsigned short* lib_feat, const unsigned char* lib_void, const int* lib_groups, long n, long plane,
                                   const unsigned short* query_feat, const unsigned short* query_mask, const int* query_groups,
                                   long n_queries, int k, int* neighbours_out, long long* distances_out, int* found_out, void* workspace,
                                   long workspace_bytes, void* stream) {
  if (!lib_feat || !lib_void || !query_feat || !query_mask || !neighbours_out || !distances_out || !found_out || !workspace) return -2;
  if ((((unsigned long long)lib_feat | (unsigned long long)query_feat | (unsigned long long)query_mask) & 15) ||
      (((unsigned long long)distances_out | (unsigned long long)workspace) & 7) ||
      (((unsigned long long)lib_groups | (unsigned long long)query_groups | (unsigned long long)neighbours_out | (unsigned long long)found_out) & 3))
    return -2;
  if (n < 1 || n > RD_AN_MAXN || plane < 1 || plane > RD_AN_MAXP || n_queries < 1 || n_queries > RD_AN_MAXQ || k < 1 || k > RD_AN_MAXK) return -2;
  // the slices: as many lists per query as the workspace holds, at most one slice per block of 64 days
  const long nblocks = rd_an_blocks(n);
  const long held = rd_pass_units(workspace_bytes, rd_an_list_bytes(n_queries, k), nblocks, nblocks);
  if (held < 1) return -2;
  const long per_slice = (nblocks + held - 1) / held, slices = (nblocks + per_slice - 1) / per_slice;
  const int C = (int)(rd_an_ppad(plane) / 8), QT = rd_an_query_tile(plane);
  const size_t lds = rd_an_lds_bytes(plane);
  const dim3 grid((unsigned)slices, (unsigned)((n_queries + QT - 1) / QT));
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* lists = (unsigned long long*)workspace;
  if (QT == RD_AN_QT_SMALL) {
    RD_TRY(ensure_lds(nullptr, (const void*)k_analog_search<RD_AN_QT_SMALL>, (size_t)RD_AN_QT_SMALL * RD_AN_QT_SPLIT * 4));
    hipLaunchKernelGGL(k_analog_search<RD_AN_QT_SMALL>, grid, dim3(RD_AN_THREADS), lds, st, (const uint4*)lib_feat, lib_void, lib_groups,
                       (const uint4*)query_feat, (const uint4*)query_mask, query_groups, (int)n, (int)n_queries, C, k, (int)nblocks,
                       (int)per_slice, lists);
  } else {
    RD_TRY(ensure_lds(nullptr, (const void*)k_analog_search<RD_AN_QT_LARGE>, (size_t)RD_AN_QT_LARGE * RD_AN_MAXP * 4));
    hipLaunchKernelGGL(k_analog_search<RD_AN_QT_LARGE>, grid, dim3(RD_AN_THREADS), lds, st, (const uint4*)lib_feat, lib_void, lib_groups,
                       (const uint4*)query_feat, (const uint4*)query_mask, query_groups, (int)n, (int)n_queries, C, k, (int)nblocks,
                       (int)per_slice, lists);
  }
  hipLaunchKernelGGL(k_analog_merge, dim3((unsigned)n_queries), dim3(64), 0, st, (const unsigned long long*)lists, slices * RD_AN_WAVES, k,
                     neighbours_out, distances_out, found_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_analog_apply(const float* lib, long n, long day_stride, long ny, long nx, const float* cond, long n_queries,
                                  long first_query, const int* neighbours, const int* found, int k, int n_members, long first_member,
                                  unsigned long long seed, int weights, float* out, int* picks_out, void* stream) {
  if (!lib || !cond || !neighbours || !found || !out || !picks_out) return -2;
  if (((unsigned long long)lib | (unsigned long long)cond | (unsigned long long)neighbours | (unsigned long long)found | (unsigned long long)out |
       (unsigned long long)picks_out) & 3)
    return -2;
  if (n < 1 || n > RD_AN_MAXN || !rd_an_shape_ok(ny, nx) || n_queries < 1 || n_queries > RD_AN_MAXQ || k < 1 || k > RD_AN_MAXK) return -2;
  const long plane = ny * nx;
  if (!rd_day_stride_ok(n, day_stride, RD_HOURS * plane) || n_members < 1 || n_members > RD_AN_MAXS) return -2;
  if (first_query < 0 || first_query > (1L << 32) - n_queries || first_member < 0 || first_member > (1L << 62)) return -2;
  if (weights != RD_AN_UNIFORM && weights != RD_AN_RANK) return -2;
  hipLaunchKernelGGL(k_analog_apply, dim3((unsigned)n_queries, (unsigned)n_members), dim3(RD_AN_APPLY_THREADS), (size_t)plane * 4,
                     (hipStream_t)stream, lib, n, day_stride, (int)plane, cond, first_query, neighbours, found, k, first_member, seed, weights,
                     out, picks_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// joint-field scores (rdgan_mvscore.hip.h): the sums of the energy score and the tables of the variogram score
// ------------------------------------------------------------------------------------
static bool rd_mv_shape_ok(long m, long D, long ny, long nx, int shared) { return rd_ensemble_shape_ok(m, D, ny, nx, shared, RD_MV_MAXM, RD_MV_MAXDAYS, 0); }
// workgroups of the largest launch of an energy call
static long rd_mv_energy_blocks(long m, long n_days, int shared) {
  if (!shared) return n_days * rd_mv_tile_pairs(rd_mv_tiles(m + 1));
  return std::max<long>((1 + n_days) * rd_mv_tile_pairs(rd_mv_tiles(m)), rd_mv_tiles(m) * rd_mv_tiles(n_days));
}
static bool rd_mv_variogram_ok(int radius, int max_lag) { return radius >= 0 && radius <= RD_MV_MAXR && max_lag >= 0 && max_lag <= RD_MV_MAXLAG; }

extern "C" long rdgan_mv_energy_workspace_bytes(long m, long n_days, int shared) {
  if (!rd_mv_shape_ok(m, n_days, 1, 1, shared) || rd_mv_energy_blocks(m, n_days, shared) > RD_MV_MAXBLOCKS) return -2;
  return rd_mv_energy_words(m, n_days, shared) * 8;
}

extern "C" int rdgan_mv_energy(const float* ens, const float* obs, long m, long n_days, long ny, long nx, int shared, double* obs_sum_out,
                               double* pair_sum_out, void* workspace, long workspace_bytes, void* stream) {
  if (!ens || !obs || !obs_sum_out || !pair_sum_out || !workspace) return -2;
  if (!rd_aligned(3, ens, obs) || !rd_aligned(7, obs_sum_out, pair_sum_out, workspace)) return -2;
  if (!rd_mv_shape_ok(m, n_days, ny, nx, shared) || rd_mv_energy_blocks(m, n_days, shared) > RD_MV_MAXBLOCKS) return -2;
  if (workspace_bytes < rd_mv_energy_words(m, n_days, shared) * 8) return -2;
  const long P = RD_HOURS * ny * nx;
  hipStream_t st = (hipStream_t)stream;
  long long* nvalid = (long long*)workspace;
  double* slots = (double*)workspace + n_days;
  hipLaunchKernelGGL(k_mv_valid, dim3((unsigned)n_days), dim3(RD_MV_THREADS), 0, st, obs, P, nvalid);
  if (!shared) {
    const long T = rd_mv_tiles(m + 1), NT = rd_mv_tile_pairs(T);
    hipLaunchKernelGGL(k_mv_energy<false>, dim3((unsigned)(n_days * NT)), dim3(RD_MV_THREADS), 0, st, ens, m * P, obs, (int)m, n_days, P, 1, 0,
                       (const long long*)nvalid, slots);
    hipLaunchKernelGGL(k_mv_energy_reduce, dim3((unsigned)n_days), dim3(RD_MV_THREADS), 0, st, (const double*)slots, (const double*)nullptr, NT,
                       (int)T, 0L, 0, P, (const long long*)nvalid, obs_sum_out, pair_sum_out);
  } else {
    const long T = rd_mv_tiles(m), NT = rd_mv_tile_pairs(T), TD = rd_mv_tiles(n_days);
    double* obs_slots = slots + (1 + n_days) * NT;
    hipLaunchKernelGGL(k_mv_energy<false>, dim3((unsigned)((1 + n_days) * NT)), dim3(RD_MV_THREADS), 0, st, ens, 0L, obs, (int)m, n_days, P, 0, 1,
                       (const long long*)nvalid, slots);
    hipLaunchKernelGGL(k_mv_energy<true>, dim3((unsigned)(T * TD)), dim3(RD_MV_THREADS), 0, st, ens, 0L, obs, (int)m, n_days, P, 0, 0,
                       (const long long*)nvalid, obs_slots);
    hipLaunchKernelGGL(k_mv_energy_reduce, dim3((unsigned)n_days), dim3(RD_MV_THREADS), 0, st, (const double*)slots, (const double*)obs_slots, NT,
                       (int)T, TD * RD_MV_TILE, 1, P, (const long long*)nvalid, obs_sum_out, pair_sum_out);
  }
  return (int)hipGetLastError();
}

extern "C" long rdgan_mv_variogram_workspace_bytes(long n_days, long ny, long nx, int radius, int max_lag, int shared) {
  if (!rd_mv_shape_ok(1, n_days, ny, nx, shared) || !rd_mv_variogram_ok(radius, max_lag)) return -2;
  if (n_days > RD_MV_MAXBLOCKS / std::max<long>(rd_mv_units(ny, nx, radius, max_lag), 1)) return -2;
  return rd_mv_variogram_words(n_days, ny, nx, radius, max_lag, shared) * 8;
}

template <bool HALF>
static void rd_mv_variogram_launch(const float* ens, const float* obs, long m, long n_days, long ny, long nx, int shared, int R, int L,
                                   double* table, rd_mv_slot* slots, hipStream_t st) {
  const long U = rd_mv_units(ny, nx, R, L), P = RD_HOURS * ny * nx;
  if (U == 0) return;                                                      // radius 0 and no lag: no displacement at all
  if (!shared) {
    hipLaunchKernelGGL((k_mv_variogram<0, HALF>), dim3((unsigned)(n_days * U)), dim3(RD_MV_THREADS), 0, st, ens, m * P, obs, (int)m, (int)ny,
                       (int)nx, R, L, table, slots);
  } else {
    hipLaunchKernelGGL((k_mv_variogram<1, HALF>), dim3((unsigned)U), dim3(RD_MV_THREADS), 0, st, ens, 0L, obs, (int)m, (int)ny, (int)nx, R, L,
                       table, slots);
    hipLaunchKernelGGL((k_mv_variogram<2, HALF>), dim3((unsigned)(n_days * U)), dim3(RD_MV_THREADS), 0, st, ens, 0L, obs, (int)m, (int)ny,
                       (int)nx, R, L, table, slots);
  }
}

extern "C" int rdgan_mv_variogram(const float* ens, const float* obs, long m, long n_days, long ny, long nx, int shared, double p, int radius,
                                  int max_lag, double* sq_out, long long* count_out, void* workspace, long workspace_bytes, void* stream) {
  if (!ens || !obs || !sq_out || !count_out || !workspace) return -2;
  if (!rd_aligned(3, ens, obs) || !rd_aligned(7, sq_out, count_out, workspace)) return -2;
  if (!rd_mv_shape_ok(m, n_days, ny, nx, shared) || !rd_mv_variogram_ok(radius, max_lag) || !(p == 0.5 || p == 1.0)) return -2;
  const long U = rd_mv_units(ny, nx, radius, max_lag);
  if (n_days > RD_MV_MAXBLOCKS / std::max<long>(U, 1) || workspace_bytes < rd_mv_variogram_words(n_days, ny, nx, radius, max_lag, shared) * 8) return -2;
  hipStream_t st = (hipStream_t)stream;
  long long* nvalid = (long long*)workspace;
  rd_mv_slot* slots = (rd_mv_slot*)((long long*)workspace + n_days);
  double* table = (double*)(slots + n_days * U * RD_MV_VG);
  hipLaunchKernelGGL(k_mv_valid, dim3((unsigned)n_days), dim3(RD_MV_THREADS), 0, st, obs, RD_HOURS * ny * nx, nvalid);
  if (p == 0.5)
    rd_mv_variogram_launch<true>(ens, obs, m, n_days, ny, nx, shared, radius, max_lag, table, slots, st);
  else
    rd_mv_variogram_launch<false>(ens, obs, m, n_days, ny, nx, shared, radius, max_lag, table, slots, st);
  const long entries = n_days * (max_lag + 1) * rd_mv_side(radius) * rd_mv_side(radius);
  hipLaunchKernelGGL(k_mv_variogram_reduce, dim3((unsigned)((entries + RD_MV_THREADS - 1) / RD_MV_THREADS)), dim3(RD_MV_THREADS), 0, st,
                     (const rd_mv_slot*)slots, n_days, (int)ny, (int)nx, radius, max_lag, (const long long*)nvalid, sq_out, count_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// log-spectral distance (rdgan_spectral.hip.h)
// ------------------------------------------------------------------------------------
extern "C" int rdgan_spectra_bins(int nd) {
  if (nd < 8 || nd > RD_SPEC_MAXND || nd % 2) return -2;
  return rd_spec_bin(nd - 1, nd - 1) - 1;               // bins 1 .. max - 1: the first and the last group are dropped
}

extern "C" int rdgan_radial_spectra(const float* fields, float* out, long n, int nd, int log_out, void* stream) {
  const int K = rdgan_spectra_bins(nd);
  if (!fields || !out || n < 1 || n > (1L << 26) || K < 1) return -2;
  rd_spec_args a;
  memset(&a, 0, sizeof(a));
  rd_twiddles(nd, -1.0, a.tw_re, a.tw_im);
  for (int i = 0; i < nd; ++i)
    for (int j = 0; j < nd; ++j) {
      const int b = rd_spec_bin(2 * j - (nd - 1), 2 * i - (nd - 1));
      if (b >= 1 && b <= K) a.cnt[b - 1]++;
    }
  for (int b = 0; b < K; ++b)
    if (a.cnt[b] == 0) return -2;
  hipStream_t st = (hipStream_t)stream;
  const int lo = log_out ? 1 : 0;
  switch (nd) {
#define RD_SPEC_CASE(ND)                                                                                                     \
  case ND: {                                                                                                                 \
    constexpr int FPB = ND * ND >= 256 ? 1 : 256 / (ND * ND);                                                                \
    hipLaunchKernelGGL(k_radial_spectra<ND>, dim3((unsigned)((n + FPB - 1) / FPB)), dim3(256), 0, st, fields, out, (int)n, K, \
                       lo, a);                                                                                               \
    break;                                                                                                                   \
  }
    RD_SPEC_CASE(8) RD_SPEC_CASE(16) RD_SPEC_CASE(24) RD_SPEC_CASE(32) RD_SPEC_CASE(48) RD_SPEC_CASE(64)
#undef RD_SPEC_CASE
    default: return -2;
  }
  return (int)hipGetLastError();
}

static void rd_lsd_grid(long n, long m, int* gx, int* gy) {
  const long nti = (n + RD_LSD_TILE - 1) / RD_LSD_TILE, ntj = (m + RD_LSD_TILE - 1) / RD_LSD_TILE;
  *gy = (int)nti;
  *gx = (int)std::max(1L, std::min(ntj, (2048 + nti - 1) / nti));     // ~2048 workgroups; a function of (n, m) alone
}

extern "C" long rdgan_lsd_workspace_bytes(long n, long m) {
  if (n < 1 || m < 1 || n > RD_LSD_MAXROWS || m > RD_LSD_MAXROWS) return -2;
  int gx, gy;
  rd_lsd_grid(n, m, &gx, &gy);
  return (long)gx * gy * (long)sizeof(rd_lsd_partial);
}

extern "C" int rdgan_lsd_pairwise(const float* spec_a, const float* spec_b, long n, long m, int k, int exclude_diagonal,
                                  float* dist, unsigned long long* hist, int nbins, float lo, float hi, double* moments,
                                  void* workspace, long workspace_bytes, void* stream) {
  if (!spec_a || !spec_b || n < 1 || m < 1 || n > RD_LSD_MAXROWS || m > RD_LSD_MAXROWS || k < 1 || k > RD_SPEC_MAXK) return -2;
  if (!dist && !hist && !moments) return -2;
  long lds = 2L * k * RD_LSD_TILE * (long)sizeof(float);
  float scale = 0.f;
  if (hist) {
    if (nbins < 1 || !(lo < hi) || !std::isfinite(lo) || !std::isfinite(hi)) return -2;
    scale = (float)nbins / (hi - lo);
    if (!std::isfinite(scale)) return -2;
    lds += 4L * (nbins + 4);
  }
  if (lds > RD_LSD_MAX_DYN_LDS) return -2;
  int gx, gy;
  rd_lsd_grid(n, m, &gx, &gy);
  if (moments && (!workspace || workspace_bytes < rdgan_lsd_workspace_bytes(n, m))) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (hist) {
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(unsigned long long) * (nbins + 4), st);
    if (e != hipSuccess) return (int)e;
  }
  rd_lsd_partial* part = moments ? (rd_lsd_partial*)workspace : nullptr;
  hipLaunchKernelGGL(k_lsd_pairwise, dim3(gx, gy), dim3(256), (size_t)lds, st, spec_a, spec_b, (int)n, (int)m, k,
                     exclude_diagonal ? 1 : 0, dist, hist, nbins, lo, hi, scale, part);
  if (moments) hipLaunchKernelGGL(k_lsd_reduce, dim3(1), dim3(256), 0, st, part, gx * gy, moments);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// RainFARM baseline (rdgan_rainfarm.hip.h)
// ------------------------------------------------------------------------------------
extern "C" int rdgan_rainfarm_classes(int nd) {
  if (!rd_rf_nd_ok(nd)) return -2;
  return (nd / 2 + 1) * (nd / 2 + 1) + RD_RF_TCLASS;
}

static void rd_rf_stat_grid(long n, int* gs, int* gt) {
  *gs = (int)std::min((long)RD_RF_STAT_WG, n * RD_RF_NT);
  *gt = (int)std::min((long)RD_RF_STAT_WG, n);
}

extern "C" long rdgan_rainfarm_stats_workspace_bytes(long n, int nd) {
  if (!rd_rf_nd_ok(nd) || n < 1 || n > RD_RF_MAXN) return -2;
  int gs, gt;
  rd_rf_stat_grid(n, &gs, &gt);
  const long nc = (long)(nd / 2 + 1) * (nd / 2 + 1);
  return ((long)gs * nc + (long)gt * RD_RF_TCLASS) * (long)sizeof(rd_rf_stat);
}

extern "C" int rdgan_rainfarm_slope_stats(const float* samples, long n, int nd, unsigned long long* counts, double* sums,
                                          void* workspace, long workspace_bytes, void* stream) {
  if (!samples || !counts || !sums || !workspace || ((uintptr_t)samples & 15)) return -2;
  const long need = rdgan_rainfarm_stats_workspace_bytes(n, nd);
  if (need < 0 || workspace_bytes < need) return -2;
  rd_rf_slope_args a;
  memset(&a, 0, sizeof(a));
  rd_twiddles(nd, -1.0, a.tw_re, a.tw_im);
  rd_twiddles(RD_RF_NT, -1.0, a.t24_re, a.t24_im);
  int gs, gt;
  rd_rf_stat_grid(n, &gs, &gt);
  const int nc = (nd / 2 + 1) * (nd / 2 + 1);
  rd_rf_stat* ps = (rd_rf_stat*)workspace;
  rd_rf_stat* pt = ps + (long)gs * nc;
  hipStream_t st = (hipStream_t)stream;
  const long nplanes = n * RD_RF_NT;
  switch (nd) {
#define RD_RF_STATS_CASE(ND)                                                                                                 \
  case ND:                                                                                                                   \
    hipLaunchKernelGGL(k_rf_spatial_stats<ND>, dim3(gs), dim3(256), 0, st, samples, nplanes, ps, a);                        \
    hipLaunchKernelGGL(k_rf_temporal_stats<ND>, dim3(gt), dim3(256), 0, st, samples, n, pt, a);                             \
    break;
    RD_RF_STATS_CASE(8) RD_RF_STATS_CASE(16) RD_RF_STATS_CASE(24) RD_RF_STATS_CASE(32) RD_RF_STATS_CASE(48) RD_RF_STATS_CASE(64)
#undef RD_RF_STATS_CASE
    default: return -2;
  }
  hipLaunchKernelGGL(k_rf_stats_reduce, dim3((nc + 255) / 256), dim3(256), 0, st, ps, gs, nc, counts, sums);
  hipLaunchKernelGGL(k_rf_stats_reduce, dim3(1), dim3(256), 0, st, pt, gt, RD_RF_TCLASS, counts + nc, sums + nc);
  return (int)hipGetLastError();
}

extern "C" long rdgan_rainfarm_gen_workspace_bytes(long n) {
  if (n < 1 || n > RD_RF_MAXN) return -2;
  return n * RD_RF_NT * (long)sizeof(float2);
}

extern "C" int rdgan_rainfarm_generate(const float* amplitudes, const float* precip, int precip_per_member, const void* uniforms,
                                       int uniforms_fp64, uint64_t seed, long first_member, float* out, long n, int nd,
                                       void* workspace, long workspace_bytes, void* stream) {
  if (!rd_rf_nd_ok(nd) || !amplitudes || !precip || !out || !workspace || first_member < 0) return -2;
  const long need = rdgan_rainfarm_gen_workspace_bytes(n);
  if (need < 0 || workspace_bytes < need || ((uintptr_t)amplitudes & 7)) return -2;
  rd_rf_gen_args a;
  memset(&a, 0, sizeof(a));
  rd_twiddles(nd, 1.0, a.tw_re, a.tw_im);
  rd_twiddles(RD_RF_NT, 1.0, a.t24_re, a.t24_im);
  const int usrc = uniforms ? (uniforms_fp64 ? 2 : 1) : 0;
  const uint32_t key = rd_make_key(seed, RD_STREAM_RAINFARM);
  const float2* amp = (const float2*)amplitudes;
  float2* stats = (float2*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)(n * RD_RF_NT);
  switch (nd) {
#define RD_RF_GEN_CASE(ND)                                                                                                   \
  case ND: {                                                                                                                 \
    constexpr int NT = rd_rf_gen_shape<ND>::NT;                                                                              \
    if (usrc == 0)                                                                                                           \
      hipLaunchKernelGGL((k_rf_gen_planes<ND, 0>), dim3(nb), dim3(NT), 0, st, amp, uniforms, key, first_member, out, stats, a); \
    else if (usrc == 1)                                                                                                      \
      hipLaunchKernelGGL((k_rf_gen_planes<ND, 1>), dim3(nb), dim3(NT), 0, st, amp, uniforms, key, first_member, out, stats, a); \
    else                                                                                                                     \
      hipLaunchKernelGGL((k_rf_gen_planes<ND, 2>), dim3(nb), dim3(NT), 0, st, amp, uniforms, key, first_member, out, stats, a); \
    hipLaunchKernelGGL(k_rf_gen_finish<ND>, dim3((unsigned)n), dim3(NT), 0, st, out, precip, precip_per_member ? 1 : 0, stats); \
    break;                                                                                                                   \
  }
    RD_RF_GEN_CASE(8) RD_RF_GEN_CASE(16) RD_RF_GEN_CASE(24) RD_RF_GEN_CASE(32) RD_RF_GEN_CASE(48) RD_RF_GEN_CASE(64)
#undef RD_RF_GEN_CASE
    default: return -2;
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// random-cascade baseline (rdgan_cascade.hip.h): the splits of wet boxes counted, and applied to daily sums
// ------------------------------------------------------------------------------------
// the edges as the kernels compare them: integers per hour, strictly increasing in 1 .. RD_CS_MAXEDGE; no edge needs no list
static bool rd_cs_edges_ok(const int* edge_units, int n_edges, rd_cs_edges* out) {
  if (n_edges < 0 || n_edges > RD_CS_MAXE || (n_edges > 0 && !edge_units)) return false;
  memset(out, 0, sizeof(*out));
  out->n = n_edges;
  for (int i = 0; i < n_edges; ++i) {
    if (edge_units[i] < 1 || edge_units[i] > RD_CS_MAXEDGE || (i > 0 && edge_units[i] <= edge_units[i - 1])) return false;
    out->v[i] = edge_units[i];
  }
  return true;
}

static bool rd_cs_shape_ok(long ny, long nx) { return ny >= 1 && nx >= 1 && ny <= RD_HOURLY_MAXPLANE && nx <= RD_HOURLY_MAXPLANE && ny * nx <= RD_HOURLY_MAXPLANE; }

extern "C" long rdgan_cascade_state_size(int n_edges) {
  if (n_edges < 0 || n_edges > RD_CS_MAXE) return -2;
  return rd_cs_state_size(n_edges);
}

extern "C" int rdgan_cascade_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, const int* edge_units, int n_edges,
                                        long long* state_inout, void* stream) {
  rd_cs_edges e;
  if (!hourly || !state_inout || !rd_aligned(7, state_inout) || !rd_aligned(3, edge_units)) return -2;
  if (!rd_cs_shape_ok(ny, nx) || !rd_cs_edges_ok(edge_units, n_edges, &e)) return -2;
  const long plane = ny * nx;
  if (!rd_hourly_layout_ok(hourly, n, day_stride, RD_HOURS * plane)) return -2;
  // a counter of a workgroup grows by at most 12 per pixel-day: 12 * 2^40 / (24 * RD_CS_ACC_MAXBLOCKS) stays below 2^32
  static_assert(12 * (RD_HOURLY_MAXELEMS / RD_HOURS / RD_CS_ACC_MAXBLOCKS + RD_CS_THREADS * 4) < (1L << 32), "32-bit LDS counters");
  const bool vec = rd_vec4_ok(hourly, plane, day_stride);
  const long items = n * (vec ? plane / 4 : plane);
  const unsigned blocks = (unsigned)std::min<long>((items + RD_CS_THREADS - 1) / RD_CS_THREADS, RD_CS_ACC_MAXBLOCKS);
  const size_t lds = (size_t)rd_cs_state_size(n_edges) * sizeof(unsigned);
  if (vec)
    hipLaunchKernelGGL(k_cascade_accumulate<4>, dim3(blocks), dim3(RD_CS_THREADS), lds, (hipStream_t)stream, hourly, n, day_stride, plane, e,
                       (unsigned long long*)state_inout);
  else
    hipLaunchKernelGGL(k_cascade_accumulate<1>, dim3(blocks), dim3(RD_CS_THREADS), lds, (hipStream_t)stream, hourly, n, day_stride, plane, e,
                       (unsigned long long*)state_inout);
  return (int)hipGetLastError();
}

extern "C" int rdgan_cascade_generate(const unsigned* model, const int* edge_units, int n_edges, const float* cond, long n_queries,
                                      long first_query, long ny, long nx, int n_members, long first_member, unsigned long long seed,
                                      int patch, float* out, int* units_out, void* stream) {
  rd_cs_edges e;
  if (!model || !cond || !out || !rd_aligned(3, model, edge_units, cond, out, units_out)) return -2;
  if (!rd_cs_shape_ok(ny, nx) || !rd_cs_edges_ok(edge_units, n_edges, &e)) return -2;
  if (n_queries < 1 || n_queries > RD_CS_MAXQ || n_members < 1 || n_members > RD_CS_MAXS || patch < 1 || patch > RD_HOURLY_MAXPLANE) return -2;
  if (first_query < 0 || first_query > (1L << 32) - n_queries || first_member < 0 || first_member > (1L << 62)) return -2;
  const long plane = ny * nx;
  if (n_queries * n_members > RD_HOURLY_MAXELEMS / (RD_HOURS * plane)) return -2;
  const bool vec = nx % 4 == 0 && rd_aligned(15, out, units_out);
  const long items = n_queries * n_members * (vec ? plane / 4 : plane);
  const unsigned blocks = (unsigned)std::min<long>((items + RD_CS_THREADS - 1) / RD_CS_THREADS, RD_CS_GEN_MAXBLOCKS);
  const size_t lds = (size_t)RD_CS_PER_CLASS * (n_edges + 1) * sizeof(unsigned);
  const int nbx = (int)((nx + patch - 1) / patch);
  if (vec)
    hipLaunchKernelGGL(k_cascade_generate<4>, dim3(blocks), dim3(RD_CS_THREADS), lds, (hipStream_t)stream, model, e, cond, n_queries, first_query,
                       (int)nx, plane, (long)n_members, first_member, seed, patch, nbx, out, units_out);
  else
    hipLaunchKernelGGL(k_cascade_generate<1>, dim3(blocks), dim3(RD_CS_THREADS), lds, (hipStream_t)stream, model, e, cond, n_queries, first_query,
                       (int)nx, plane, (long)n_members, first_member, seed, patch, nbx, out, units_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// extremes of hourly fields (rdgan_extremes.hip.h): block maxima of the k-hour depths per pixel, L-moment sums of series of maxima
// ------------------------------------------------------------------------------------
// the window mask of the peak kernels (rd_peaks_mask): bit w - 1 for a window of w hours, 1 .. RD_EX_MAXK windows of 1 .. 24 hours
static bool rd_ex_mask_ok(unsigned mask) { return mask != 0u && mask < (1u << RD_HOURS) && __builtin_popcount(mask) <= RD_EX_MAXK; }

// the days of a workgroup's run where the caller leaves the choice: about 2048 workgroups, and RD_EX_MINRUN days at least
static long rd_ex_run(long n, long groups) {
  const long even = (n * groups + 2047) / 2048;
  return std::min<long>(n, std::min<long>(RD_EX_MAXRUN, std::max<long>(RD_EX_MINRUN, even)));
}

extern "C" int rdgan_block_maxima_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, const int* block, long n_blocks,
                                             unsigned window_mask, int days_per_run, long long* bmax_inout, int* ndays_inout,
                                             int* nvoid_inout, void* stream) {
  if (!hourly || !block || !bmax_inout || !ndays_inout || !nvoid_inout) return -2;
  if (!rd_aligned(7, bmax_inout) || !rd_aligned(3, ndays_inout, nvoid_inout) || !rd_ar_shape_ok(ny, nx)) return -2;
  if (!rd_ex_mask_ok(window_mask) || n_blocks < 1 || n_blocks > RD_EX_MAXBLOCKS || days_per_run < 0 || days_per_run > RD_EX_MAXRUN) return -2;
  const long plane = ny * nx, K = __builtin_popcount(window_mask);
  if (n_blocks > RD_EX_MAXSTATE / (K * plane)) return -2;
  if (!rd_hourly_layout_ok(hourly, n, day_stride, RD_HOURS * plane)) return -2;
  for (long d = 0; d < n; ++d)
    if (block[d] < 0 || block[d] >= n_blocks) return -2;
  const bool vec = rd_vec4_ok(hourly, plane, day_stride);
  const long groups = ((vec ? plane / 4 : plane) + RD_EX_THREADS - 1) / RD_EX_THREADS;
  const long run = days_per_run ? std::min<long>(days_per_run, n) : rd_ex_run(n, groups);
  const long runs = (n + run - 1) / run;
  if (runs > 0x7FFFFFFFL / groups) return -2;                              // (only a days_per_run far below the array's size)
  hipStream_t st = (hipStream_t)stream;
  int* dev = nullptr;
  RD_TRY(rd_field_upload(block, (size_t)n, &dev, st));
  if (vec)
    hipLaunchKernelGGL(k_block_maxima<4>, dim3((unsigned)(groups * runs)), dim3(RD_EX_THREADS), 0, st, hourly, n, day_stride, plane,
                       (const int*)dev, n_blocks, window_mask, (int)run, groups, bmax_inout, ndays_inout, nvoid_inout);
  else
    hipLaunchKernelGGL(k_block_maxima<1>, dim3((unsigned)(groups * runs)), dim3(RD_EX_THREADS), 0, st, hourly, n, day_stride, plane,
                       (const int*)dev, n_blocks, window_mask, (int)run, groups, bmax_inout, ndays_inout, nvoid_inout);
  hipError_t e = hipGetLastError();
  hipError_t f = hipFreeAsync(dev, st);
  return (int)(e != hipSuccess ? e : f);
}

extern "C" int rdgan_lmoment_sums(const long long* table, const int* ndays, int min_days, long n_series, int n_blocks, long n_positions,
                                  long long* sums_out, int* n_out, long long* sorted_out, void* stream) {
  if (!table || !sums_out || !n_out || !rd_aligned(7, table, sums_out, sorted_out) || !rd_aligned(3, ndays, n_out)) return -2;
  if (n_series < 1 || n_positions < 1 || n_blocks < 1 || n_blocks > RD_EX_MAXB) return -2;
  if (n_positions > RD_HOURLY_MAXELEMS / n_blocks || n_series > RD_HOURLY_MAXELEMS / (n_blocks * n_positions)) return -2;
  const long tiles = n_series * ((n_positions + RD_EX_PX - 1) / RD_EX_PX);
  RD_TRY(ensure_lds(nullptr, (const void*)k_lmoment_sums, RD_EX_LDS_MAX));
  hipLaunchKernelGGL(k_lmoment_sums, dim3((unsigned)std::min<long>(tiles, 1L << 20)), dim3(RD_EX_THREADS),
                     RD_EX_LDS_HEAD + (size_t)n_blocks * RD_EX_PX * sizeof(long long), (hipStream_t)stream, table, ndays, min_days, n_series,
                     n_blocks, n_positions, sums_out, n_out, sorted_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// chaining scenarios across midnight (rdgan_sequence.hip.h): edge features, seam costs, the min-plus step and the greedy matching
// ------------------------------------------------------------------------------------
static bool rd_seq_shape_ok(long s, long n_days, long plane) {
  return s >= 1 && s <= RD_SEQ_MAXS && n_days >= 1 && n_days <= RD_SEQ_MAXDAYS && plane >= 1 && plane <= RD_HOURLY_MAXPLANE;
}

extern "C" long rdgan_seq_workspace_bytes(long n_members, long n_boundaries) {
  if (n_members < 1 || n_members > RD_SEQ_MAXS || n_boundaries < 1 || n_boundaries > RD_SEQ_MAXDAYS) return -2;
  return n_boundaries * rd_seq_match_bytes(n_members);
}

extern "C" int rdgan_seq_edges(const float* hourly, long n, long day_stride, long ny, long nx, long n_days, int first_hour, int last_hour,
                               unsigned short* feat_out, unsigned int* bad_inout, void* stream) {
  if (!hourly || !feat_out || !bad_inout || !rd_aligned(15, feat_out) || !rd_aligned(3, bad_inout)) return -2;
  if (ny < 1 || nx < 1 || ny > RD_HOURLY_MAXPLANE || nx > RD_HOURLY_MAXPLANE || ny * nx > RD_HOURLY_MAXPLANE) return -2;
  if (first_hour < 0 || first_hour >= RD_HOURS || last_hour < 0 || last_hour >= RD_HOURS) return -2;
  const long plane = ny * nx;
  if (n_days < 1 || n_days > RD_SEQ_MAXDAYS || !rd_hourly_layout_ok(hourly, n, day_stride, RD_HOURS * plane) || n % n_days != 0) return -2;
  if (n / n_days > RD_SEQ_MAXS) return -2;
  const int U = (int)(rd_seq_ppad(plane) / 8), W = (int)rd_seq_words(plane);
  const long blocks = (n * 2 * U + 255) / 256;
  if (blocks > 0x7FFFFFFFL) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (rd_vec4_ok(hourly, plane, day_stride))
    hipLaunchKernelGGL(k_seq_edges<true>, dim3((unsigned)blocks), dim3(256), 0, st, hourly, n, day_stride, (int)plane, U, W, n_days, first_hour,
                       last_hour, (uint4*)feat_out, bad_inout);
  else
    hipLaunchKernelGGL(k_seq_edges<false>, dim3((unsigned)blocks), dim3(256), 0, st, hourly, n, day_stride, (int)plane, U, W, n_days, first_hour,
                       last_hour, (uint4*)feat_out, bad_inout);
  return (int)hipGetLastError();
}

extern "C" int rdgan_seq_costs(const unsigned short* feat_a, const unsigned int* bad_a, long s_a, const unsigned short* feat_b,
                               const unsigned int* bad_b, long s_b, long n_days, long plane, int shift, int pixel_splits,
                               long long* costs_out, long long* n_valid_out, void* stream) {
  if (!feat_a || !bad_a || !feat_b || !bad_b || !costs_out || !n_valid_out) return -2;
  if (!rd_aligned(15, feat_a, feat_b) || !rd_aligned(3, bad_a, bad_b) || !rd_aligned(7, costs_out, n_valid_out)) return -2;
  if (!rd_seq_shape_ok(s_a, n_days, plane) || !rd_seq_shape_ok(s_b, n_days, plane) || shift < 0 || shift >= n_days) return -2;
  const long B = n_days - shift;
  if (B * s_a * s_b > RD_SEQ_MAXCOSTS || pixel_splits < 0) return -2;
  const int U = (int)(rd_seq_ppad(plane) / 8), W = (int)rd_seq_words(plane);
  const long TA = rd_seq_tiles(s_a), TB = rd_seq_tiles(s_b), nchunks = (U + RD_SEQ_CHUNK - 1) / RD_SEQ_CHUNK;
  // the pixel chunks are cut into pixel_splits ranges, or, left to the entry (0), into as many as bring the launch to about
  // RD_SEQ_TARGET_BLOCKS workgroups; never more than there are chunks
  long nsplit = std::min<long>(nchunks, pixel_splits ? pixel_splits : std::max<long>(1, (RD_SEQ_TARGET_BLOCKS + B * TA * TB - 1) / (B * TA * TB)));
  const long per_split = (nchunks + nsplit - 1) / nsplit;
  nsplit = (nchunks + per_split - 1) / per_split;
  if (B * TA * TB * nsplit > 0x7FFFFFFFL) return -2;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY((int)hipMemsetAsync(costs_out, 0, (size_t)(B * s_a * s_b) * 8, st));
  hipLaunchKernelGGL(k_seq_valid, dim3((unsigned)B), dim3(256), 0, st, bad_a, bad_b, W, shift, plane, n_valid_out);
  hipLaunchKernelGGL(k_seq_costs, dim3((unsigned)(B * TA * TB * nsplit)), dim3(RD_SEQ_THREADS), 0, st, (const uint4*)feat_a, bad_a, (int)s_a,
                     (const uint4*)feat_b, bad_b, (int)s_b, n_days, U, W, shift, (int)TA, (int)TB, (int)nsplit, (int)per_split,
                     (unsigned long long*)costs_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_seq_minplus(const long long* costs, long n_boundaries, long n_members, long long* acc_out, int* back_out, void* stream) {
  if (!costs || !acc_out || !back_out || !rd_aligned(7, costs, acc_out) || !rd_aligned(3, back_out)) return -2;
  if (n_members < 1 || n_members > RD_SEQ_MAXS || n_boundaries < 1 || n_boundaries > RD_SEQ_MAXDAYS) return -2;
  if (n_boundaries * n_members * n_members > RD_SEQ_MAXCOSTS) return -2;
  const long S = n_members;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY((int)hipMemsetAsync(acc_out, 0, (size_t)S * 8, st));
  for (long b = 0; b < n_boundaries; ++b)
    hipLaunchKernelGGL(k_seq_minplus, dim3((unsigned)((S + 63) / 64)), dim3(256), 0, st, costs + b * S * S, (int)S,
                       (const long long*)(acc_out + b * S), acc_out + (b + 1) * S, back_out + b * S);
  return (int)hipGetLastError();
}

extern "C" int rdgan_seq_match(const long long* costs, long n_boundaries, long n_members, int init, int rounds, int* perm_inout,
                               int* free_rows_inout, void* workspace, long workspace_bytes, void* stream) {
  if (!costs || !perm_inout || !free_rows_inout || !workspace) return -2;
  if (!rd_aligned(7, costs, workspace) || !rd_aligned(3, perm_inout, free_rows_inout)) return -2;
  if (n_members < 1 || n_members > RD_SEQ_MAXS || n_boundaries < 1 || n_boundaries > RD_SEQ_MAXDAYS) return -2;
  if (n_boundaries * n_members * n_members > RD_SEQ_MAXCOSTS) return -2;
  if ((init != 0 && init != 1) || rounds < 0 || rounds > RD_SEQ_MAXS || workspace_bytes < n_boundaries * rd_seq_match_bytes(n_members)) return -2;
  const int S = (int)n_members;
  const dim3 per_member((unsigned)((S + 255) / 256), (unsigned)n_boundaries), per_rows((unsigned)((S + RD_SEQ_ROWS - 1) / RD_SEQ_ROWS), (unsigned)n_boundaries);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_seq_match_init, per_member, dim3(256), 0, st, S, init, perm_inout, free_rows_inout, workspace);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(k_seq_match_minima, per_rows, dim3(RD_SEQ_THREADS), 0, st, costs, S, r & 1, (const int*)free_rows_inout, workspace);
    hipLaunchKernelGGL(k_seq_match_take, per_member, dim3(256), 0, st, S, r & 1, perm_inout, free_rows_inout, workspace);
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// least-cost assignment of the members of neighbouring days (rdgan_assign.hip.h): one workgroup solves one boundary
// ------------------------------------------------------------------------------------
extern "C" int rdgan_assign(const long long* costs, long n_boundaries, long n_members, int* perm_out, long long* u_out, long long* v_out,
                            long long* total_out, void* stream) {
  if (!costs || !perm_out || !u_out || !v_out || !total_out) return -2;
  if (!rd_aligned(7, costs, u_out, v_out, total_out) || !rd_aligned(3, perm_out)) return -2;
  if (n_members < 1 || n_members > RD_SEQ_MAXS || n_boundaries < 1 || n_boundaries > RD_SEQ_MAXDAYS) return -2;
  if (n_boundaries * n_members * n_members > RD_SEQ_MAXCOSTS) return -2;
  hipLaunchKernelGGL(k_seq_assign, dim3((unsigned)n_boundaries), dim3(RD_ASG_THREADS), 0, (hipStream_t)stream, costs, (int)n_members, perm_out,
                     u_out, v_out, total_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// scenario reduction (rdgan_reduce.hip.h): pooled features, all-pairs distances, forward selection and assignment
// ------------------------------------------------------------------------------------
// Pf of a member, or 0 for a shape outside the limits
static long rd_red_positions(long n_days, long ny, long nx, long pool) {
  if (pool != 1 && pool != 2 && pool != 4 && pool != RD_RED_MAXPOOL) return 0;
  if (n_days < 1 || ny < 1 || nx < 1 || ny > RD_HOURLY_MAXPLANE || nx > RD_HOURLY_MAXPLANE || ny * nx > RD_HOURLY_MAXPLANE) return 0;
  if (n_days > RD_HOURLY_MAXELEMS / (RD_HOURS * ny * nx)) return 0;
  return n_days * RD_HOURS * rd_red_blocks(ny, pool) * rd_red_blocks(nx, pool);
}
// Pf 65535 S < 2^52: a row sum of distances, shifted by 12, stays inside 64 bits
static bool rd_red_admit(long s, long n_positions) {
  return s >= 1 && s <= RD_RED_MAXS && n_positions >= 1 && n_positions <= ((1L << RD_RED_KEYBITS) - 1) / ((long)RD_SEQ_FEATMAX * s);
}

extern "C" long rdgan_red_workspace_bytes(long n_members, long k) {
  if (n_members < 1 || n_members > RD_RED_MAXS || k < 1 || k > n_members) return -2;
  return rd_red_select_bytes(n_members, k);
}

extern "C" int rdgan_red_features(const float* hourly, long n_members, long member_stride, long n_days, long ny, long nx, int pool,
                                  unsigned short* feat_out, long feat_stride, unsigned int* bad_inout, void* stream) {
  if (!hourly || !feat_out || !bad_inout || !rd_aligned(15, feat_out) || !rd_aligned(3, bad_inout)) return -2;
  const long Pf = rd_red_positions(n_days, ny, nx, pool);
  if (Pf < 1 || !rd_red_admit(n_members, Pf)) return -2;
  if (!rd_hourly_layout_ok(hourly, n_members, member_stride, n_days * RD_HOURS * ny * nx)) return -2;
  const long Ppad = rd_seq_ppad(Pf), U = Ppad / 8;
  if (feat_stride % 8 != 0 || !rd_day_stride_ok(n_members, feat_stride, Ppad)) return -2;
  const long blocks = (n_members * U + 255) / 256;
  if (blocks > 0x7FFFFFFFL) return -2;
  const int by = (int)rd_red_blocks(ny, pool), bx = (int)rd_red_blocks(nx, pool);
  hipStream_t st = (hipStream_t)stream;
  if (pool == 1 && rd_aligned(15, hourly) && member_stride % 4 == 0)
    hipLaunchKernelGGL(k_red_features<true>, dim3((unsigned)blocks), dim3(256), 0, st, hourly, n_members, member_stride, Pf, (int)ny, (int)nx, pool,
                       by, bx, U, (uint4*)feat_out, feat_stride / 8, bad_inout);
  else
    hipLaunchKernelGGL(k_red_features<false>, dim3((unsigned)blocks), dim3(256), 0, st, hourly, n_members, member_stride, Pf, (int)ny, (int)nx, pool,
                       by, bx, U, (uint4*)feat_out, feat_stride / 8, bad_inout);
  return (int)hipGetLastError();
}

extern "C" int rdgan_red_distances(const unsigned short* feat, const unsigned int* bad, long n_members, long feat_stride, long n_positions,
                                   int position_splits, long long* dist_out, long long* n_valid_out, void* stream) {
  if (!feat || !bad || !dist_out || !n_valid_out) return -2;
  if (!rd_aligned(15, feat) || !rd_aligned(3, bad) || !rd_aligned(7, dist_out, n_valid_out)) return -2;
  if (!rd_red_admit(n_members, n_positions) || position_splits < 0) return -2;
  const long Ppad = rd_seq_ppad(n_positions), U = Ppad / 8, W = rd_seq_words(n_positions), S = n_members;
  if (feat_stride % 8 != 0 || !rd_day_stride_ok(S, feat_stride, Ppad)) return -2;
  const long T = rd_seq_tiles(S), tiles = rd_red_tri(T), nchunks = (U + RD_SEQ_CHUNK - 1) / RD_SEQ_CHUNK;
  // the chunks of positions are cut into position_splits ranges, or, left to the entry (0), into as many as bring the launch to about
  // RD_RED_TARGET_BLOCKS workgroups; never more than there are chunks
  long nsplit = std::min<long>(nchunks, position_splits ? position_splits : std::max<long>(1, (RD_RED_TARGET_BLOCKS + tiles - 1) / tiles));
  const long per_split = (nchunks + nsplit - 1) / nsplit;
  nsplit = (nchunks + per_split - 1) / per_split;
  if (tiles * nsplit > 0x7FFFFFFFL) return -2;
  hipStream_t st = (hipStream_t)stream;
  RD_TRY((int)hipMemsetAsync(dist_out, 0, (size_t)(S * S) * 8, st));
  RD_TRY((int)hipMemsetAsync(n_valid_out, 0, 8, st));
  hipLaunchKernelGGL(k_red_valid, dim3((unsigned)std::min<long>((W + 255) / 256, 1024)), dim3(256), 0, st, bad, W, n_positions,
                     (unsigned long long*)n_valid_out);
  hipLaunchKernelGGL(k_red_distances, dim3((unsigned)(tiles * nsplit)), dim3(RD_SEQ_THREADS), 0, st, (const uint4*)feat, bad, (int)S, feat_stride / 8,
                     U, (int)T, (int)nsplit, per_split, (unsigned long long*)dist_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_red_select(const long long* dist, long n_members, long k, int* chosen_out, long long* cost_out, int* assign_out,
                                int* counts_out, void* workspace, long workspace_bytes, void* stream) {
  if (!dist || !chosen_out || !cost_out || !assign_out || !counts_out || !workspace) return -2;
  if (!rd_aligned(7, dist, cost_out, workspace) || !rd_aligned(3, chosen_out, assign_out, counts_out)) return -2;
  if (n_members < 1 || n_members > RD_RED_MAXS || k < 1 || k > n_members || workspace_bytes < rd_red_select_bytes(n_members, k)) return -2;
  const int S = (int)n_members;
  unsigned long long* m = (unsigned long long*)workspace;
  unsigned long long* slot = m + S;
  unsigned char* selected = (unsigned char*)(slot + k);
  hipStream_t st = (hipStream_t)stream;
  RD_TRY((int)hipMemsetAsync(m, 0xFF, (size_t)(S + k) * 8, st));           // m = +inf, every slot empty
  RD_TRY((int)hipMemsetAsync(selected, 0, (size_t)S, st));
  RD_TRY((int)hipMemsetAsync(counts_out, 0, (size_t)k * 4, st));
  RD_TRY((int)hipMemsetAsync(chosen_out, 0xFF, (size_t)k * 4, st));
  const dim3 per_rows((unsigned)((S + RD_RED_ROWS - 1) / RD_RED_ROWS)), per_member((unsigned)((S + 255) / 256));
  for (long t = 0; t < k; ++t) {
    hipLaunchKernelGGL(k_red_select, per_rows, dim3(256), 0, st, dist, S, (const unsigned long long*)m, (const unsigned char*)selected, slot + t);
    hipLaunchKernelGGL(k_red_update, per_member, dim3(256), 0, st, dist, S, (const unsigned long long*)(slot + t), m, selected,
                       chosen_out + t, cost_out + t);
  }
  hipLaunchKernelGGL(k_red_assign, per_member, dim3(256), 0, st, dist, S, (int)k, (const int*)chosen_out, assign_out, counts_out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// multivariate rank histograms (rdgan_mvrank.hip.h): the sums behind the average-rank and band-depth pre-ranks, leave-one-out MST lengths
// ------------------------------------------------------------------------------------
// N = m + 1 vectors (the observation and the members) of 24 ny nx values: N 24 ny nx within RD_HOURLY_MAXELEMS
static bool rd_mvr_shape_ok(long m, long D, long ny, long nx, int shared) { return rd_ensemble_shape_ok(m, D, ny, nx, shared, RD_MVR_MAXM, RD_MVR_MAXDAYS, 1); }

// nothing is kept between the launches of a call today: the size is the least a caller may pass
extern "C" long rdgan_mvr_ranks_workspace_bytes(long m, long n_days, int shared) {
  if (!rd_mvr_shape_ok(m, n_days, 1, 1, shared)) return -2;
  return 8;
}

template <int TP>
static int rd_mvr_ranks_launch(const float* ens, const float* obs, long N, long n_days, long P, int shared, int position_runs,
                               long long* sums_out, long long* n_valid_out, hipStream_t st) {
  const long planes = n_days * RD_HOURS, tiles = (P + TP - 1) / TP;
  // the tiles of a plane are cut into position_runs runs, or, left to the entry (0), into as many as bring the launch to about
  // RD_MVR_TARGET_BLOCKS workgroups; never more than there are tiles
  long runs = std::min<long>(tiles, position_runs ? position_runs : std::max<long>(1, (RD_MVR_TARGET_BLOCKS + planes - 1) / planes));
  const long per_run = (tiles + runs - 1) / runs;
  runs = (tiles + per_run - 1) / per_run;
  if (planes * runs > 0x7FFFFFFFL) return -2;
  const size_t lds = (size_t)rd_mvr_lds_bytes(N);
  RD_TRY(ensure_lds(nullptr, (const void*)k_mvr_ranks<TP>, lds));
  RD_TRY((int)hipMemsetAsync(sums_out, 0, (size_t)(planes * N * 2) * 8, st));
  RD_TRY((int)hipMemsetAsync(n_valid_out, 0, (size_t)planes * 8, st));
  hipLaunchKernelGGL(k_mvr_ranks<TP>, dim3((unsigned)(planes * runs)), dim3(RD_MVR_THREADS), lds, st, ens, obs, (int)N,
                     shared ? 0L : (N - 1) * RD_HOURS * P, P, tiles, (int)runs, per_run, (unsigned long long*)sums_out,
                     (unsigned long long*)n_valid_out);
  return (int)hipGetLastError();
}

extern "C" int rdgan_mvr_ranks(const float* ens, const float* obs, long m, long n_days, long ny, long nx, int shared, int position_runs,
                               long long* sums_out, long long* n_valid_out, void* workspace, long workspace_bytes, void* stream) {
  if (!ens || !obs || !sums_out || !n_valid_out || !workspace) return -2;
  if (!rd_aligned(3, ens, obs) || !rd_aligned(7, sums_out, n_valid_out, workspace)) return -2;
  if (!rd_mvr_shape_ok(m, n_days, ny, nx, shared) || position_runs < 0 || workspace_bytes < 8) return -2;
  const long N = m + 1, P = ny * nx;
  hipStream_t st = (hipStream_t)stream;
  switch (rd_mvr_tp(N)) {
    case 64: return rd_mvr_ranks_launch<64>(ens, obs, N, n_days, P, shared, position_runs, sums_out, n_valid_out, st);
    case 32: return rd_mvr_ranks_launch<32>(ens, obs, N, n_days, P, shared, position_runs, sums_out, n_valid_out, st);
    case 16: return rd_mvr_ranks_launch<16>(ens, obs, N, n_days, P, shared, position_runs, sums_out, n_valid_out, st);
    default: return rd_mvr_ranks_launch<8>(ens, obs, N, n_days, P, shared, position_runs, sums_out, n_valid_out, st);
  }
}

extern "C" int rdgan_mvr_mst(const long long* dist, long n, long long* len_out, void* stream) {
  if (!dist || !len_out || !rd_aligned(7, dist, len_out) || n < 1 || n > RD_MVR_MAXN) return -2;
  hipLaunchKernelGGL(k_mvr_mst, dim3((unsigned)n), dim3(RD_MVR_THREADS), 0, (hipStream_t)stream, dist, (int)n, len_out);
  return (int)hipGetLastError();
}
