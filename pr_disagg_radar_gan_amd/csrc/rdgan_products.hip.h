// Ensemble products of whole fields: per-pixel k-hour peaks of hourly maps, formed where the hours already
// pass through registers, and statistics across the members of an ensemble.
//
//  * k_hourly_peaks: x [units][24][ny][nx] -> peaks [units][K][ny][nx], peak_hour [units][ny][nx] (uint8).  For the windows
//    win[0] < win[1] < .. < win[K - 1] (each 1 .. 24, handed over as the bit mask sum 1 << (win - 1)):
//      peaks[u][i][y][x] = max over h0 = 0 .. 24 - win[i] of v[h0] + v[h0 + 1] + .. + v[h0 + win[i] - 1]
//    summed in fp32 from left to right, every add rounded; peak_hour = the FIRST h0 reaching the maximum of win[0].  The maximum is
//    taken with `>` from h0 = 0 on, so a later equal sum (or a NaN one, inf - inf) never replaces an earlier one.  A pixel with a
//    NaN among its 24 hours gives NaN for every window and hour 255.
//  * k_field_blend_peaks: the inputs of k_field_blend (rdgan_field.hip.h), the outputs of k_hourly_peaks.  The 24 hourly values of
//    a pixel are formed by the SAME device functions k_field_blend calls (rd_field_resolve, rd_field_hour) and reduced by the one
//    k_hourly_peaks calls (rd_window_peaks), so the result equals k_hourly_peaks(k_field_blend(..)) bit for bit and the hourly
//    planes are never written.  A dry pixel gives 0 and hour 0, a NaN pixel NaN and 255; neither reads frac.
//  * k_member_stats: x[s * member_stride + p], s < S members, p < P positions -> per position Q quantiles (numpy "linear", fp64,
//    rounded once), the mean (fp64 sum in a fixed order) and T exceedance frequencies #{x > thr} / S.  A workgroup takes a run of
//    PX adjacent positions, so every member row is read in segments of PX * 4 contiguous bytes, and sorts the PX columns side by
//    side in LDS with the bitonic network of rd_dist_load_sort (rdgan_dist.hip.h), padded to NP = pow2(S) with +inf.
//    LDS layout xs[i][px] (member index outer, position inner), NOT xs[px][i]: ds_read_b32 / ds_write_b32 serve a wave in two groups
//    of 32 lanes over 32 banks of 4 bytes.  With px innermost the 32 lanes of a group hold 32 consecutive dwords in the load (which
//    is also the contiguous global read), in both operands of every compare-exchange (lanes differ in px, or in px and the low bits
//    of i, never in a multiple of 32 dwords) and in the binary searches behind the sort, where every lane probes a different index
//    `mid` of its own column: address mid * PX + px falls into bank px mod 32 whatever mid is (PX = 16: two-way at worst, PX = 8:
//    four-way).  With i innermost a column's stride NP is a multiple of 32 dwords, so the load would hit one bank 32 times over and
//    the searches would collide at random.
// No floating-point atomics anywhere; sums run in a fixed order: two calls agree bit for bit.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_field.hip.h"
#include "rdgan_dist.hip.h"

#define RD_PEAKS_MAXK 8

// The k-hour peaks of one pixel from its 24 hourly values in registers.  pk points at the pixel in the first of the K = popcount(mask)
// output planes, `plane` apart; hr at its peak hour.  Every index into v and s is a compile-time constant (no scratch): window w is
// reached by adding hour h0 + w - 1 to the running sum s[h0] of window w - 1, which IS the left-to-right sum of the definition.
__device__ __forceinline__ void rd_window_peaks(const float (&v)[RD_HOURS], unsigned mask, int w0, float* __restrict__ pk,
                                                long plane, unsigned char* __restrict__ hr) {
#pragma clang fp contract(off)
  bool nan = false;
#pragma unroll
  for (int h = 0; h < RD_HOURS; ++h) nan |= v[h] != v[h];
  float s[RD_HOURS];
  int hour = 0;
  long k = 0;
#pragma unroll
  for (int w = 1; w <= RD_HOURS; ++w) {
    if ((mask >> (w - 1)) == 0u) break;                  // no window of w hours or more is asked for
#pragma unroll
    for (int h0 = 0; h0 + w <= RD_HOURS; ++h0) s[h0] = w == 1 ? v[h0] : s[h0] + v[h0 + w - 1];
    if ((mask >> (w - 1)) & 1u) {
      float best = s[0];
      int bh = 0;
#pragma unroll
      for (int h0 = 1; h0 + w <= RD_HOURS; ++h0)
        if (s[h0] > best) {
          best = s[h0];
          bh = h0;
        }
      pk[k * plane] = nan ? __builtin_nanf("") : best;
      if (w == w0) hour = bh;
      ++k;
    }
  }
  *hr = (unsigned char)(nan ? 255 : hour);
}

// The thread layout of k_field_blend: a workgroup takes a 4 x 64 patch of one unit, lane = x; a wave reads 64 contiguous floats of
// each of the 24 planes and writes 64 contiguous floats of each of the K planes and 64 contiguous bytes.
__global__ void __launch_bounds__(RD_FIELD_THREADS)
k_hourly_peaks(const float* __restrict__ x, long units, int ny, int nx, unsigned mask, int w0, float* __restrict__ peaks,
               unsigned char* __restrict__ peak_hour) {
#pragma clang fp contract(off)
  const int lx = threadIdx.x & (RD_FIELD_BX - 1), ly = threadIdx.x / RD_FIELD_BX;
  const long plane = (long)ny * nx, K = __popc(mask);
  const long nbx = (nx + RD_FIELD_BX - 1) / RD_FIELD_BX, nby = (ny + RD_FIELD_BY - 1) / RD_FIELD_BY;
  const long n_blocks = units * nby * nbx;
  for (long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const long u = b / (nby * nbx);
    const int y = (int)((b / nbx) % nby) * RD_FIELD_BY + ly, xx = (int)(b % nbx) * RD_FIELD_BX + lx;
    if (y >= ny || xx >= nx) continue;
    const long pix = (long)y * nx + xx;
    const float* src = x + u * RD_HOURS * plane + pix;
    float v[RD_HOURS];
#pragma unroll
    for (int h = 0; h < RD_HOURS; ++h) v[h] = src[h * plane];
    rd_window_peaks(v, mask, w0, peaks + u * K * plane + pix, plane, peak_hour + u * plane + pix);
  }
}

// k_field_blend with the window reduction in place of the 24 stores; arguments as there, peaks [units][K][ny][nx],
// peak_hour [units][ny][nx].
__global__ void __launch_bounds__(RD_FIELD_THREADS)
k_field_blend_peaks(const float* __restrict__ frac, const int* __restrict__ slots, const int* __restrict__ ytab_i,
                    const float* __restrict__ ytab_w, const int* __restrict__ xtab_i, const float* __restrict__ xtab_w,
                    const float* __restrict__ daily, float* __restrict__ peaks, unsigned char* __restrict__ peak_hour, long units,
                    long first_unit, long n_days, int ny, int nx, int nd, int step, int n_ty, int n_tx, unsigned mask, int w0) {
#pragma clang fp contract(off)
  const int lx = threadIdx.x & (RD_FIELD_BX - 1), ly = threadIdx.x / RD_FIELD_BX;
  const long plane = (long)ny * nx, tile = (long)nd * nd, K = __popc(mask);
  const int T = n_ty * n_tx;
  const long nbx = (nx + RD_FIELD_BX - 1) / RD_FIELD_BX, nby = (ny + RD_FIELD_BY - 1) / RD_FIELD_BY;
  const long n_blocks = units * nby * nbx;
  for (long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const long u = b / (nby * nbx);
    const int y = (int)((b / nbx) % nby) * RD_FIELD_BY + ly, x = (int)(b % nbx) * RD_FIELD_BX + lx;
    if (y >= ny || x >= nx) continue;
    const long pix = (long)y * nx + x;
    const float d = daily[((first_unit + u) % n_days) * plane + pix];
    float* pk = peaks + u * K * plane + pix;
    unsigned char* hr = peak_hour + u * plane + pix;
    if (d == 0.f || d != d) {
      for (long k = 0; k < K; ++k) pk[k * plane] = d;                      // 0 stays 0, NaN stays NaN
      *hr = (unsigned char)(d == 0.f ? 0 : 255);
      continue;
    }
    long off[RD_FIELD_COVER * RD_FIELD_COVER];
    float w[RD_FIELD_COVER * RD_FIELD_COVER];
    rd_field_resolve(slots + u * T, ytab_i, ytab_w, xtab_i, xtab_w, y, x, ny, nx, nd, step, n_ty, n_tx, off, w);
    float v[RD_HOURS];
#pragma unroll
    for (int h = 0; h < RD_HOURS; ++h) v[h] = rd_field_hour(frac, off, w, h, tile, d);
    rd_window_peaks(v, mask, w0, pk, plane, hr);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
#define RD_MS_THREADS 1024
#define RD_MS_MAXS 4096
#define RD_MS_MAXQ 16
#define RD_MS_MAXT 16
#define RD_MS_MAXPX 64
#define RD_MS_COL_FLOATS 32768                        // PX * pow2(S) floats of columns: 128 KiB of the CU's 160 KiB
#define RD_MS_LDS_HEAD (RD_MS_THREADS * sizeof(double) + RD_MS_MAXPX * sizeof(int))
#define RD_MS_LDS_MAX (RD_MS_LDS_HEAD + RD_MS_COL_FLOATS * sizeof(float))

struct rd_ms_args {
  double probs[RD_MS_MAXQ];
  double thr[RD_MS_MAXT];
};

// the run width for S members: as many positions as fit, a power of two, at most 64 -- 64 up to S = 512, 32 up to 1024, 16 up to
// 2048, 8 up to 4096
__host__ __device__ __forceinline__ int rd_ms_run_width(int npow2) {
  const int px = RD_MS_COL_FLOATS / npow2;
  return px < RD_MS_MAXPX ? px : RD_MS_MAXPX;
}

// 1024 threads per run of PX = 1 << lpx positions; dynamic LDS RD_MS_LDS_HEAD + NP * PX floats.
//   quant [Q][P], mean [P], exceed [T][P] (T may be 0), n_nan: one 64-bit count (cleared by the caller) of the positions holding a
//   NaN member, added with one integer atomic per run; those positions get NaN in every output.
// Thread t owns position px = t % PX in the load, the sort and the partial sums, so a wave touches 64 / PX consecutive member rows
// of PX consecutive floats.  mean: thread (g, px), g = t / PX, adds members g, g + G, g + 2G, .. (G = 1024 / PX) of its sorted column
// in fp64, then a fixed tree over g.
__global__ void __launch_bounds__(RD_MS_THREADS)
k_member_stats(const float* __restrict__ x, long member_stride, int S, int NP, int lpx, long P, int Q, int T, rd_ms_args a,
               float* __restrict__ quant, float* __restrict__ mean, float* __restrict__ exceed,
               unsigned long long* __restrict__ n_nan) {
  extern __shared__ double rd_ms_lds[];
  double* red = rd_ms_lds;
  int* flag = (int*)(red + RD_MS_THREADS);
  float* xs = (float*)(flag + RD_MS_MAXPX);
  const int t = threadIdx.x;
  const int PX = 1 << lpx, G = RD_MS_THREADS >> lpx;
  const int px = t & (PX - 1), g = t >> lpx;
  const long runs = (P + PX - 1) >> lpx;
  const int total = NP << lpx;
  for (long run = blockIdx.x; run < runs; run += gridDim.x) {
    const long p0 = run << lpx;
    const bool live = p0 + px < P;                     // (the tail run: the columns past P hold +inf and are not written)
    __syncthreads();                                   // the previous run's outputs have been formed
    if (t < PX) flag[t] = 0;
    __syncthreads();
    const float* src = x + p0 + px;
    for (int i = g; i < NP; i += G) {
      float v = (i < S && live) ? src[(long)i * member_stride] : __builtin_inff();
      if (v != v) {
        flag[px] = 1;
        v = __builtin_inff();
      }
      xs[(i << lpx) + px] = v;
    }
    __syncthreads();
    if (t == 0) {
      int c = 0;
      for (int k = 0; k < PX; ++k) c += flag[k];
      if (c) atomicAdd(n_nan, (unsigned long long)c);
    }
    // the bitonic network of rd_dist_load_sort on every column: pair r of a stage is (i, i | j), i = r with a 0 inserted at bit j
    for (int k = 2; k <= NP; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int q = t; q < (total >> 1); q += RD_MS_THREADS) {
          const int r = q >> lpx;
          const int i = ((r & ~(j - 1)) << 1) | (r & (j - 1));
          const int ia = (i << lpx) + px, ib = ((i | j) << lpx) + px;
          const float va = xs[ia], vb = xs[ib];
          const bool up = (i & k) == 0;
          if ((va > vb) == up) {
            xs[ia] = vb;
            xs[ib] = va;
          }
        }
        __syncthreads();
      }
    double s = 0.0;
    for (int i = g; i < S; i += G) s += (double)xs[(i << lpx) + px];
    red[t] = s;
    __syncthreads();
    for (int h = G >> 1; h > 0; h >>= 1) {
      if (g < h) red[t] += red[t + (h << lpx)];
      __syncthreads();
    }
    for (int task = t; task < (1 + Q + T) << lpx; task += RD_MS_THREADS) {
      const int c = task & (PX - 1), k = task >> lpx;            // (c == px: 1024 is a multiple of PX)
      const long p = p0 + c;
      if (p >= P) continue;
      const bool bad = flag[c] != 0;
      const float* col = xs + c;
      float r;
      if (k == 0) {
        r = (float)(red[c] / (double)S);
      } else if (k <= Q) {
        r = (float)rd_np_quantile(col, S, a.probs[k - 1], PX);
      } else {
        r = (float)((double)(S - rd_count_le(col, S, a.thr[k - 1 - Q], PX)) / (double)S);
      }
      if (bad) r = __builtin_nanf("");
      float* dst = k == 0 ? mean : (k <= Q ? quant + (long)(k - 1) * P : exceed + (long)(k - 1 - Q) * P);
      dst[p] = r;
    }
  }
}
