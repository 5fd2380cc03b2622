// RainFARM baseline (reference rainfarm/rainfarm_temporal_downscaling.py): the statistics behind the spectral-slope calibration
// (fp64) and the stochastic spatio-temporal generation of days from their daily sums (fp32).  DESIGN.md section 10.
#pragma once
#include "rdgan_rng.h"

#define RD_RF_NT 24                    // hours per day: the time axis of every transform here
#define RD_RF_MAXND 64
#define RD_RF_TCLASS 13                // temporal classes |m| = 0 .. 12
#define RD_RF_STAT_WG 1024             // workgroups of the two statistics kernels (fewer when there is less work)
#define RD_RF_MAXN (1L << 24)          // samples / members per call

__host__ __device__ inline bool rd_rf_nd_ok(int nd) {
  return nd == 8 || nd == 16 || nd == 24 || nd == 32 || nd == 48 || nd == 64;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Slope statistics.  Per frequency class: the number of kept points and the fp64 sum of log(|F|^2) over them.  A point is kept
// when its power is > 0 and its frequency is not zero (the reference's isfinite(log) and k != 0 / omega != 0 filters).
// ---------------------------------------------------------------------------------------------------------------------------
struct rd_rf_stat {
  double sum;
  long long cnt;
};

struct rd_rf_slope_args {
  double tw_re[RD_RF_MAXND], tw_im[RD_RF_MAXND];   // exp(-2 pi i j / nd)
  double t24_re[RD_RF_NT], t24_im[RD_RF_NT];       // exp(-2 pi i m / 24)
};

// Spatial: every hour plane of every sample.  A workgroup takes planes blockIdx.x, + gridDim.x, ...: plane into LDS, real-input row
// DFT for the columns k = 0 .. nd/2, column DFT, log power.  The columns 1 .. nd/2 - 1 stand for their conjugate mirrors too
// (same power, same class (|a|, |b|)), so they count twice.  Thread c owns classes c, c + 256, ... for the whole launch: the sums
// are in a fixed order.  As in k_radial_spectra, the nonzero frequencies are summed over x[n] - x[0] so that a constant row or
// column gives exactly zero power (dropped, as the reference's FFT drops it) instead of a rounding residue.
template <int ND>
__global__ __launch_bounds__(256) void k_rf_spatial_stats(const float* __restrict__ x, long nplanes, rd_rf_stat* __restrict__ part,
                                                          rd_rf_slope_args a) {
  constexpr int H = ND / 2 + 1, NN = ND * ND, NH = ND * H, NC = H * H, CPT = (NC + 255) / 256;
  __shared__ __attribute__((aligned(16))) double lp[NH];   // the plane (NN floats) until the row pass, then the log powers
  __shared__ double2 R[NH];
  __shared__ double2 tw[ND];
  float* xs = (float*)lp;
  const int t = threadIdx.x;
  for (int i = t; i < ND; i += 256) tw[i] = make_double2(a.tw_re[i], a.tw_im[i]);
  double csum[CPT];
  long long ccnt[CPT];
#pragma unroll
  for (int q = 0; q < CPT; ++q) { csum[q] = 0.0; ccnt[q] = 0; }
  for (long p = blockIdx.x; p < nplanes; p += gridDim.x) {
    __syncthreads();                                 // the previous plane's class pass is done with lp
    const float4* src = (const float4*)(x + p * NN);
    for (int i = t; i < NN / 4; i += 256) ((float4*)xs)[i] = src[i];
    __syncthreads();
    for (int o = t; o < NH; o += 256) {              // R[y][k] = sum_n (x[y][n] - (k ? x[y][0] : 0)) w^(k n)
      const int y = o / H, k = o % H;
      const float* row = xs + y * ND;
      const double x0 = k ? (double)row[0] : 0.0;
      double re = 0.0, im = 0.0;
      int idx = 0;
#pragma unroll
      for (int n = 0; n < ND; ++n) {
        const double v = (double)row[n] - x0;
        const double2 w = tw[idx];
        re = fma(v, w.x, re);
        im = fma(v, w.y, im);
        idx += k;
        if (idx >= ND) idx -= ND;
      }
      R[o] = make_double2(re, im);
    }
    __syncthreads();
    for (int o = t; o < NH; o += 256) {              // F[l][k] = sum_y (R[y][k] - (l ? R[0][k] : 0)) w^(l y)
      const int l = o / H, k = o % H;
      const double2 c0 = l ? R[k] : make_double2(0.0, 0.0);
      double re = 0.0, im = 0.0;
      int idx = 0;
#pragma unroll
      for (int y = 0; y < ND; ++y) {
        const double2 v = R[y * H + k];
        const double vr = v.x - c0.x, vi = v.y - c0.y;
        const double2 w = tw[idx];
        re = fma(vr, w.x, fma(-vi, w.y, re));
        im = fma(vr, w.y, fma(vi, w.x, im));
        idx += l;
        if (idx >= ND) idx -= ND;
      }
      const double pw = re * re + im * im;
      lp[o] = (pw > 0.0 && o != 0) ? log(pw) : (double)NAN;     // NaN marks a dropped point
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = t + 256 * q;
      if (c >= NC) continue;
      const int ca = c / H, cb = c % H;
      const int wgt = (cb == 0 || cb == ND / 2) ? 1 : 2;
      const double v0 = lp[ca * H + cb];
      if (v0 == v0) { csum[q] += wgt * v0; ccnt[q] += wgt; }
      if (ca != 0 && ca != ND / 2) {
        const double v1 = lp[(ND - ca) * H + cb];
        if (v1 == v1) { csum[q] += wgt * v1; ccnt[q] += wgt; }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int c = t + 256 * q;
    if (c < NC) {
      rd_rf_stat s;
      s.sum = csum[q];
      s.cnt = ccnt[q];
      part[(long)blockIdx.x * NC + c] = s;
    }
  }
}

// Temporal: the 24-point DFT of every pixel series, one pixel per thread (samples blockIdx.x, + gridDim.x, ...; pixels t, t + 256,
// ...).  Real input: m = 1 .. 11 stand for 24 - m too and count twice, m = 12 once.  Per-thread class sums, then a fixed LDS tree.
template <int ND>
__global__ __launch_bounds__(256) void k_rf_temporal_stats(const float* __restrict__ x, long n, rd_rf_stat* __restrict__ part,
                                                           rd_rf_slope_args a) {
  constexpr int NN = ND * ND;
  __shared__ double2 tw[RD_RF_NT];
  __shared__ double r_sum[256];
  __shared__ long long r_cnt[256];
  const int t = threadIdx.x;
  for (int i = t; i < RD_RF_NT; i += 256) tw[i] = make_double2(a.t24_re[i], a.t24_im[i]);
  __syncthreads();
  double s[12];
  long long c[12];
#pragma unroll
  for (int m = 0; m < 12; ++m) { s[m] = 0.0; c[m] = 0; }
  for (long smp = blockIdx.x; smp < n; smp += gridDim.x)
    for (int px = t; px < NN; px += 256) {
      const float* src = x + smp * RD_RF_NT * NN + px;
      double v[RD_RF_NT];
#pragma unroll
      for (int tau = 0; tau < RD_RF_NT; ++tau) v[tau] = (double)src[(long)tau * NN];
#pragma unroll
      for (int tau = RD_RF_NT - 1; tau >= 0; --tau) v[tau] -= v[0];
#pragma unroll
      for (int m = 1; m <= 12; ++m) {
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int tau = 1; tau < RD_RF_NT; ++tau) {
          const double2 w = tw[(m * tau) % RD_RF_NT];
          re = fma(v[tau], w.x, re);
          im = fma(v[tau], w.y, im);
        }
        const double pw = re * re + im * im;
        if (pw > 0.0) {
          const int wgt = m < 12 ? 2 : 1;
          s[m - 1] += wgt * log(pw);
          c[m - 1] += wgt;
        }
      }
    }
  rd_rf_stat* out = part + (long)blockIdx.x * RD_RF_TCLASS;
  if (t == 0) {
    rd_rf_stat z;
    z.sum = 0.0;
    z.cnt = 0;
    out[0] = z;                                      // m = 0 is never kept
  }
#pragma unroll
  for (int m = 0; m < 12; ++m) {
    __syncthreads();
    r_sum[t] = s[m];
    r_cnt[t] = c[m];
    for (int h = 128; h > 0; h >>= 1) {
      __syncthreads();
      if (t < h) { r_sum[t] += r_sum[t + h]; r_cnt[t] += r_cnt[t + h]; }
    }
    if (t == 0) {
      rd_rf_stat z;
      z.sum = r_sum[0];
      z.cnt = r_cnt[0];
      out[m + 1] = z;
    }
  }
}

// counts[c] / sums[c] = the partials of class c added in workgroup order: bit-identical on every call.
__global__ __launch_bounds__(256) void k_rf_stats_reduce(const rd_rf_stat* __restrict__ part, int nparts, int nclass,
                                                         unsigned long long* __restrict__ counts, double* __restrict__ sums) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nclass) return;
  double s = 0.0;
  long long k = 0;
  for (int g = 0; g < nparts; ++g) {
    const rd_rf_stat p = part[(long)g * nclass + c];
    s += p.sum;
    k += p.cnt;
  }
  counts[c] = (unsigned long long)k;
  sums[c] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Generation.  g = Re IDFT_3(A e^{2 pi i u}) up to the factor 1 / (24 nd^2), which the division by std(g) cancels.
// ---------------------------------------------------------------------------------------------------------------------------
struct rd_rf_gen_args {
  float tw_re[RD_RF_MAXND], tw_im[RD_RF_MAXND];    // exp(+2 pi i j / nd)
  float t24_re[RD_RF_NT], t24_im[RD_RF_NT];        // exp(+2 pi i m / 24)
};

template <int ND>
struct rd_rf_gen_shape {
  static constexpr int NN = ND * ND;
  static constexpr int NT = NN < 256 ? NN : 256;   // 64 threads at nd 8, 256 otherwise
  static constexpr int EPT = (NN + NT - 1) / NT;
};

template <int NT>
__device__ inline float rd_rf_block_sum(float v, float* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  for (int h = NT / 2; h > 0; h >>= 1) {
    __syncthreads();
    if (t < h) red[t] += red[t + h];
  }
  __syncthreads();
  return red[0];
}

// One workgroup per (member, hour t), blockIdx.x = 24 m + t.  (1) the time sum H_t(a, b) = sum_tau A[tau][a][b] e^{2 pi i u}
// w24^(tau t) over tau = 1 .. 23 (A is zero at tau = 0), one (a, b) per thread, the phase by sincospi of 2u (2u in [0, 2): no
// range reduction error); (2) row IDFT H -> R in LDS; (3) column IDFT, real part only -> g into out; the plane's mean and sum of
// squared deviations (fixed LDS trees) -> stats[24 m + t].  USRC: 0 counter RNG, 1 fp32 uniforms, 2 fp64 uniforms ([n][24 nd^2]).
template <int ND, int USRC>
__global__ __launch_bounds__(rd_rf_gen_shape<ND>::NT) void k_rf_gen_planes(const float2* __restrict__ amp, const void* __restrict__ uni,
                                                                           uint32_t base_key, long first_member, float* __restrict__ out,
                                                                           float2* __restrict__ stats, rd_rf_gen_args a) {
#pragma clang fp contract(off)   // no fusing left to the compiler: the three phase sources run the same arithmetic, bit for bit
  constexpr int NN = rd_rf_gen_shape<ND>::NN, NT = rd_rf_gen_shape<ND>::NT, EPT = rd_rf_gen_shape<ND>::EPT;
  __shared__ float2 Hs[NN], Rs[NN];
  __shared__ float2 tw[ND], t24[RD_RF_NT];
  __shared__ float red[NT];
  const int tid = threadIdx.x;
  const long m = blockIdx.x / RD_RF_NT;
  const int t = blockIdx.x % RD_RF_NT;
  for (int i = tid; i < ND; i += NT) tw[i] = make_float2(a.tw_re[i], a.tw_im[i]);
  for (int i = tid; i < RD_RF_NT; i += NT) t24[i] = make_float2(a.t24_re[i], a.t24_im[i]);
  const uint32_t key = USRC == 0 ? rd_member_key(base_key, (uint64_t)(first_member + m)) : 0u;
  const long ubase = m * RD_RF_NT * NN;
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < EPT; ++q) {
    const int e2 = tid + q * NT;
    if (e2 >= NN) break;
    float hr = 0.f, hi = 0.f;
    int idx = 0;
    for (int tau = 1; tau < RD_RF_NT; ++tau) {
      idx += t;
      if (idx >= RD_RF_NT) idx -= RD_RF_NT;
      const int e = tau * NN + e2;
      float d;                                     // 2u, reduced to [-1, 1) where that is exact
      if (USRC == 0) {
        d = 2.f * rd_uniform(key, (uint32_t)e);
      } else if (USRC == 1) {
        d = 2.f * ((const float*)uni)[ubase + e];
      } else {
        const double dd = 2.0 * ((const double*)uni)[ubase + e];
        d = (float)(dd >= 1.0 ? dd - 2.0 : dd);
      }
      float s, c;
      sincospif(d, &s, &c);
      const float2 A = amp[e];
      const float pr = fmaf(A.x, c, -(A.y * s)), pim = fmaf(A.x, s, A.y * c);
      const float2 w = t24[idx];
      hr = fmaf(pr, w.x, fmaf(-pim, w.y, hr));
      hi = fmaf(pr, w.y, fmaf(pim, w.x, hi));
    }
    Hs[e2] = make_float2(hr, hi);
  }
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < EPT; ++q) {                  // R[a][j] = sum_b H[a][b] w^(b j)
    const int o = tid + q * NT;
    if (o >= NN) break;
    const int ra = o / ND, j = o % ND;
    const float2* row = Hs + ra * ND;
    float re = 0.f, im = 0.f;
    int idx = 0;
#pragma unroll
    for (int b = 0; b < ND; ++b) {
      const float2 h = row[b], w = tw[idx];
      re = fmaf(h.x, w.x, fmaf(-h.y, w.y, re));
      im = fmaf(h.x, w.y, fmaf(h.y, w.x, im));
      idx += j;
      if (idx >= ND) idx -= ND;
    }
    Rs[o] = make_float2(re, im);
  }
  __syncthreads();
  float* gs = (float*)Hs;                          // H is dead after the row pass: the plane of g, for the statistics
  float lsum = 0.f;
  float* dst = out + (m * RD_RF_NT + t) * NN;
#pragma unroll 1
  for (int q = 0; q < EPT; ++q) {                  // g[i][j] = Re sum_a R[a][j] w^(a i)
    const int o = tid + q * NT;
    if (o >= NN) break;
    const int i = o / ND, j = o % ND;
    float g = 0.f;
    int idx = 0;
#pragma unroll
    for (int ra = 0; ra < ND; ++ra) {
      const float2 r = Rs[ra * ND + j], w = tw[idx];
      g = fmaf(r.x, w.x, fmaf(-r.y, w.y, g));
      idx += i;
      if (idx >= ND) idx -= ND;
    }
    gs[o] = g;
    lsum += g;
    dst[o] = g;
  }
  const float mean = rd_rf_block_sum<NT>(lsum, red) * (1.f / (float)NN);
  float lsq = 0.f;
  for (int o = tid; o < NN; o += NT) {             // (each thread reads back its own values: no barrier needed before this)
    const float dv = gs[o] - mean;
    lsq = fmaf(dv, dv, lsq);
  }
  const float m2 = rd_rf_block_sum<NT>(lsq, red);
  if (tid == 0) stats[blockIdx.x] = make_float2(mean, m2);
}

// One workgroup per member: the day's population std from its 24 plane statistics (equal counts: grand mean = mean of the means,
// M2 = sum M2_t + NN sum (mean_t - mean)^2, in hour order), then per pixel r_t = exp(g_t / std), out_t = r_t precip / sum_t r_t.
// The exponent is shifted by the pixel's largest g_t / std (the ratio is unchanged; exp cannot overflow).  precip 0 gives exact 0.
template <int ND>
__global__ __launch_bounds__(rd_rf_gen_shape<ND>::NT) void k_rf_gen_finish(float* __restrict__ out, const float* __restrict__ precip,
                                                                           int precip_per_member, const float2* __restrict__ stats) {
#pragma clang fp contract(off)
  constexpr int NN = rd_rf_gen_shape<ND>::NN, NT = rd_rf_gen_shape<ND>::NT;
  const long m = blockIdx.x;
  const float2* st = stats + m * RD_RF_NT;
  float mean = 0.f;
  for (int t = 0; t < RD_RF_NT; ++t) mean += st[t].x;
  mean *= 1.f / (float)RD_RF_NT;
  float m2 = 0.f;
  for (int t = 0; t < RD_RF_NT; ++t) {
    const float d = st[t].x - mean;
    m2 += st[t].y + (float)NN * d * d;
  }
  const float inv = 1.f / sqrtf(m2 / (float)(RD_RF_NT * NN));
  const float* pr = precip + (precip_per_member ? m * NN : 0L);
  float* day = out + m * RD_RF_NT * NN;
  for (int px = threadIdx.x; px < NN; px += NT) {
    float z[RD_RF_NT];
    float zmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < RD_RF_NT; ++t) {
      z[t] = day[t * NN + px] * inv;
      zmax = fmaxf(zmax, z[t]);
    }
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < RD_RF_NT; ++t) {
      z[t] = expf(z[t] - zmax);
      s += z[t];
    }
    const float f = pr[px] / s;
#pragma unroll
    for (int t = 0; t < RD_RF_NT; ++t) day[t * NN + px] = z[t] * f;
  }
}
