// The CRPS experiment's own kernels: the "random" climatological baseline of
// generate_and_evaluate_crps.py:164, 193-194 -- MANY observed days scored against ONE fixed ensemble -- and the statistics of
// analyze_crps_results.py (moments for the one-sample t-test, :14; the bootstrapped means, :25-35).
//
//  * k_crps_fixed: crps = mean_i |x_i - y| - 0.5 mean_{i,j} |x_i - x_j| per grid point.  The spread term does not depend on y, and
//    with the members sorted, P_k the sum of the k smallest and k = #{x_i <= y}:
//        mean_i |x_i - y| = ( y (2k - n) - 2 P_k + P_n ) / n
//    so the members of a grid point are sorted ONCE (the bitonic network of k_crps_ensemble, rdgan_data.hip.h), an fp64 prefix
//    table is built beside the sorted column in LDS, and every day costs one binary search.  The three terms cancel at large n,
//    hence the prefix sums and the expression in fp64; the result is rounded to fp32 once.
//  * k_crps_hourly: the area mean per (day, hour) of :191, fp64 in a fixed order.
//  * k_bootstrap_means: resampled means, indices from the counter RNG (rdgan_rng.h, RD_STREAM_BOOTSTRAP).
//  * k_moments_f64: count, mean, unbiased variance, two passes.
// Every sum here runs in a fixed order (per-thread strides, then a fixed LDS tree or scan): no floating-point atomics, and two calls
// agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_rng.h"

#define RD_CRPS_THREADS 1024
#define RD_CRPS_MAXN 8192

// sum of one value per thread over a 1024-thread block, fixed tree in LDS; every thread gets the result.  red: 1024 doubles.
__device__ __forceinline__ double rd_block_sum_f64(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();                                    // (red may still be read from a previous use)
  red[t] = v;
  __syncthreads();
  for (int s = RD_CRPS_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// One 1024-thread block per grid point p.  Dynamic LDS: pre[n + 1] doubles (P_0 .. P_n), red[1024] doubles, xs[npow2] floats.
// ens [n][npos], obs [D][npos], crps [D][npos].  A NaN observation gives NaN; members must be finite.
__global__ void __launch_bounds__(RD_CRPS_THREADS)
k_crps_fixed(const float* __restrict__ ens, const float* __restrict__ obs, float* __restrict__ crps, int n, int npow2, long n_days,
             long npos) {
  extern __shared__ double rd_crps_lds[];
  double* pre = rd_crps_lds;
  double* red = pre + (n + 1);
  float* xs = (float*)(red + RD_CRPS_THREADS);
  const int t = threadIdx.x;
  const long p = blockIdx.x;
  for (int i = t; i < npow2; i += RD_CRPS_THREADS) xs[i] = i < n ? ens[(long)i * npos + p] : __builtin_inff();
  __syncthreads();
  for (int k = 2; k <= npow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npow2; i += RD_CRPS_THREADS) {
        int l = i ^ j;
        if (l > i) {
          float a = xs[i], b = xs[l];
          bool up = (i & k) == 0;
          if ((a > b) == up) { xs[i] = b; xs[l] = a; }
        }
      }
      __syncthreads();
    }
  // prefix sums: thread t owns the contiguous members [t c, (t + 1) c); a scan of the 1024 chunk sums gives its offset
  const int c = (n + RD_CRPS_THREADS - 1) / RD_CRPS_THREADS;
  const int i0 = min(t * c, n), i1 = min(i0 + c, n);
  double s_chunk = 0.0, s_spread = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double x = (double)xs[i];
    s_chunk += x;
    s_spread += (double)(2 * i + 1 - n) * x;           // sum_{i<j} (x_(j) - x_(i)) = sum_i (2i - n - 1) x_(i), i = 1..n
  }
  red[t] = s_chunk;
  __syncthreads();
  for (int off = 1; off < RD_CRPS_THREADS; off <<= 1) {
    const double v = t >= off ? red[t - off] : 0.0;
    __syncthreads();
    red[t] += v;
    __syncthreads();
  }
  double run = t > 0 ? red[t - 1] : 0.0;               // the sum of every member in front of i0
  if (t == 0) pre[0] = 0.0;
  for (int i = i0; i < i1; ++i) {
    run += (double)xs[i];
    pre[i + 1] = run;
  }
  const double dn = (double)n;
  const double spread = rd_block_sum_f64(s_spread, red) / (dn * dn);      // 0.5 mean_{i,j} |x_i - x_j|
  const double p_n = pre[n];                           // (published by the barriers inside rd_block_sum_f64)
  for (long d = t; d < n_days; d += RD_CRPS_THREADS) {
    const float y = obs[d * npos + p];
    int lo = 0, hi = n;                                // k = #{x_i <= y}
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (xs[mid] <= y) lo = mid + 1; else hi = mid;
    }
    const double yd = (double)y;
    const double mabs = (yd * (double)(2 * lo - n) - 2.0 * pre[lo] + p_n) / dn;
    crps[d * npos + p] = y != y ? y : (float)(mabs - spread);
  }
}

// One 256-thread block per (day, hour): mean of the npix = nd * nd per-position values, fp64, fixed order.
__global__ void __launch_bounds__(256)
k_crps_hourly(const float* __restrict__ crps, float* __restrict__ hourly, int npix) {
  __shared__ double red[256];
  const float* src = crps + (long)blockIdx.x * npix;
  double s = 0.0;
  for (int i = threadIdx.x; i < npix; i += 256) s += (double)src[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) hourly[blockIdx.x] = (float)(red[0] / (double)npix);
}

// One 1024-thread block per resample r = first + blockIdx.x: mean of n draws x[idx(r, i)], i = 0 .. n - 1,
//   idx = (uint64(rd_bits(rd_member_key(base, r), i)) * n) >> 32,  base = rd_make_key(seed, RD_STREAM_BOOTSTRAP)
// so a draw depends on (seed, r, i) only.  Thread t sums the draws i = t, t + 1024, ... in fp64, then the fixed tree.
__global__ void __launch_bounds__(RD_CRPS_THREADS)
k_bootstrap_means(const double* __restrict__ x, uint32_t n, uint32_t base, uint64_t first, double* __restrict__ means) {
  __shared__ double red[RD_CRPS_THREADS];
  const uint32_t key = rd_member_key(base, first + blockIdx.x);
  double s = 0.0;
  for (uint64_t i = threadIdx.x; i < n; i += RD_CRPS_THREADS) {
    const uint32_t idx = (uint32_t)(((uint64_t)rd_bits(key, (uint32_t)i) * n) >> 32);
    s += x[idx];
  }
  s = rd_block_sum_f64(s, red);
  if (threadIdx.x == 0) means[blockIdx.x] = s / (double)n;
}

// One 1024-thread block: out3 = { n, mean, sum (x - mean)^2 / (n - 1) }, two passes in fp64 (n = 1: variance 0/0 = NaN, as numpy).
__global__ void __launch_bounds__(RD_CRPS_THREADS)
k_moments_f64(const double* __restrict__ x, long n, double* __restrict__ out3) {
  __shared__ double red[RD_CRPS_THREADS];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += RD_CRPS_THREADS) s += x[i];
  const double mean = rd_block_sum_f64(s, red) / (double)n;
  double q = 0.0;
  for (long i = threadIdx.x; i < n; i += RD_CRPS_THREADS) {
    const double d = x[i] - mean;
    q += d * d;
  }
  q = rd_block_sum_f64(q, red);
  if (threadIdx.x == 0) {
    out3[0] = (double)n;
    out3[1] = mean;
    out3[2] = q / (double)(n - 1);
  }
}
