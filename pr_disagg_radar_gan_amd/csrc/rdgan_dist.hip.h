// Distribution checks of generate_and_evaluate.py:431-604: the two-sample Kolmogorov-Smirnov statistic of
// :583, the box-plot statistics sns.boxplot draws at :495, :499, :600 (matplotlib.cbook.boxplot_stats, whis = 1.5) and the ECDF of
// :431-452 counted on a grid of thresholds.
//
//  * k_ks_2samp, k_box_stats: one 1024-thread block per column.  Samples lie as the reference holds them, x[batch][n][ncol]; a
//    column is the n values of one (batch, col), read with stride ncol.  The column is padded to a power of two with +inf and
//    sorted once in LDS by the bitonic network of k_crps_fixed; everything after that is a binary search or a fixed tree.
//  * k_ecdf_grid + k_ecdf_scan: any number of values in one pass; per value a binary search in the thresholds (LDS), counts in an
//    LDS histogram, merged into a global 64-bit histogram with INTEGER atomics (counts do not depend on the order of the adds),
//    then an inclusive scan.
// No floating-point atomics; every fp64 sum runs in a fixed order, so two calls agree bit for bit.  A NaN is found while the column
// is loaded (the bitonic compare does not order it) and raises a per-column flag.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_crps.hip.h"

#define RD_DIST_THREADS RD_CRPS_THREADS
#define RD_DIST_MAXN 16384
#define RD_DIST_NSTATS 12
#define RD_ECDF_THREADS 256
#define RD_ECDF_MAXT 4096
#define RD_ECDF_MAXBLOCKS 1024

// dynamic LDS of the two column kernels at the largest n (bytes); both stay inside the 160 KiB of a CDNA4 CU
#define RD_KS_LDS_HEAD (RD_DIST_THREADS * (sizeof(long long) + 2 * sizeof(int)) + 2 * sizeof(int))
#define RD_KS_LDS_MAX (RD_KS_LDS_HEAD + 2 * RD_DIST_MAXN * sizeof(float))
#define RD_BOX_LDS_HEAD (RD_DIST_THREADS * sizeof(double) + 2 * sizeof(int))
#define RD_BOX_LDS_MAX (RD_BOX_LDS_HEAD + RD_DIST_MAXN * sizeof(float))

// xs[0 .. npow2) = the column (n values, stride `stride`) padded with +inf, ascending.  A NaN sets *nan_flag and is stored as +inf.
// *nan_flag must have been cleared behind a barrier.
__device__ __forceinline__ void rd_dist_load_sort(const float* __restrict__ col, long stride, int n, int npow2, float* xs,
                                                  int* nan_flag) {
  const int t = threadIdx.x;
  for (int i = t; i < npow2; i += RD_DIST_THREADS) {
    float v = i < n ? col[(long)i * stride] : __builtin_inff();
    if (v != v) {
      *nan_flag = 1;
      v = __builtin_inff();
    }
    xs[i] = v;
  }
  __syncthreads();
  for (int k = 2; k <= npow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npow2; i += RD_DIST_THREADS) {
        int l = i ^ j;
        if (l > i) {
          float a = xs[i], b = xs[l];
          bool up = (i & k) == 0;
          if ((a > b) == up) { xs[i] = b; xs[l] = a; }
        }
      }
      __syncthreads();
    }
}

// #{ xs[i] <= v } and #{ xs[i] < v } over the ascending xs[0 .. n), element i at xs[i * stride] (columns sorted side by side in LDS,
// rdgan_products.hip.h, pass their run width)
__device__ __forceinline__ int rd_count_le(const float* xs, int n, double v, int stride = 1) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((double)xs[mid * stride] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int rd_count_lt(const float* xs, int n, double v, int stride = 1) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((double)xs[mid * stride] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// a candidate (i, j) = (#{a <= v}, #{b <= v}) beats the best so far with a larger |i m - j n| (= n m |F_a(v) - F_b(v)|, exact in
// integers), or with the same and a smaller i + j: i + j grows strictly with v, so that is the FIRST v reaching the maximum
__device__ __forceinline__ void rd_ks_take(long long& key, int& bi, int& bj, long long k2, int i2, int j2) {
  if (k2 > key || (k2 == key && i2 + j2 < bi + bj)) {
    key = k2;
    bi = i2;
    bj = j2;
  }
}

// One block per column c of batch entry bt (blockIdx.x = bt * ncol + c).  a [batch][n][ncol], b [batch][m][ncol];
// counts [batch][ncol][2] = (i, j), d [batch][ncol] = |i / n - j / m|.  F_a and F_b are compared only at the END of a run of equal
// values (all of them consumed, in both samples): thread t takes the elements p = t, t + 1024, ... of a that close a run, finds
// j = #{b <= a_p} by binary search, and likewise for b; a fixed tree takes the maximum.  Dynamic LDS: RD_KS_LDS_HEAD + (npa + npb) floats.
__global__ void __launch_bounds__(RD_DIST_THREADS)
k_ks_2samp(const float* __restrict__ a, const float* __restrict__ b, int n, int m, int npa, int npb, int ncol,
           int* __restrict__ counts, double* __restrict__ d_out) {
  extern __shared__ double rd_dist_lds[];
  long long* rkey = (long long*)rd_dist_lds;
  int* ri = (int*)(rkey + RD_DIST_THREADS);
  int* rj = ri + RD_DIST_THREADS;
  int* flag = rj + RD_DIST_THREADS;
  float* xa = (float*)(flag + 2);
  float* xb = xa + npa;
  const int t = threadIdx.x;
  const long bt = blockIdx.x / ncol, c = blockIdx.x % ncol;
  if (t == 0) *flag = 0;
  __syncthreads();
  rd_dist_load_sort(a + bt * n * ncol + c, ncol, n, npa, xa, flag);
  rd_dist_load_sort(b + bt * m * ncol + c, ncol, m, npb, xb, flag);
  long long key = -1;
  int bi = 0, bj = 0;
  for (int p = t; p < n; p += RD_DIST_THREADS)
    if (p == n - 1 || xa[p + 1] != xa[p]) {
      const int i = p + 1, j = rd_count_le(xb, m, (double)xa[p]);
      const long long k2 = (long long)i * m - (long long)j * n;
      rd_ks_take(key, bi, bj, k2 < 0 ? -k2 : k2, i, j);
    }
  for (int q = t; q < m; q += RD_DIST_THREADS)
    if (q == m - 1 || xb[q + 1] != xb[q]) {
      const int j = q + 1, i = rd_count_le(xa, n, (double)xb[q]);
      const long long k2 = (long long)i * m - (long long)j * n;
      rd_ks_take(key, bi, bj, k2 < 0 ? -k2 : k2, i, j);
    }
  rkey[t] = key;
  ri[t] = bi;
  rj[t] = bj;
  __syncthreads();
  for (int s = RD_DIST_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      rd_ks_take(key, bi, bj, rkey[t + s], ri[t + s], rj[t + s]);
      rkey[t] = key;
      ri[t] = bi;
      rj[t] = bj;
    }
    __syncthreads();
  }
  if (t == 0) {
    const bool bad = *flag != 0;
    counts[2 * (long)blockIdx.x] = bad ? -1 : bi;
    counts[2 * (long)blockIdx.x + 1] = bad ? -1 : bj;
    d_out[blockIdx.x] = bad ? __builtin_nan("") : fabs((double)bi / (double)n - (double)bj / (double)m);
  }
}

// np.percentile(x, 100 q) of the ascending xs[0 .. n), method "linear": virtual index (n - 1) q, numpy's lerp a + (b - a) g, and
// b - (b - a)(1 - g) for g >= 0.5; fp64, no contraction into FMA.  Element i lies at xs[i * stride].
__device__ __forceinline__ double rd_np_quantile(const float* xs, int n, double q, int stride = 1) {
#pragma clang fp contract(off)
  const double vi = (double)(n - 1) * q;
  const int lo = (int)floor(vi);
  const int hi = min(lo + 1, n - 1);
  const double g = vi - (double)lo;
  const double a = (double)xs[lo * stride], b = (double)xs[hi * stride];
  const double diff = b - a;
  double r = a + diff * g;
  if (g >= 0.5) r = b - diff * (1.0 - g);
  return r;
}

// One block per column.  x [batch][n][ncol]; stats [batch][ncol][12] = n, mean, q1, med, q3, iqr, whislo, whishi, cilo, cihi,
// n_fliers_lo, n_fliers_hi as matplotlib.cbook.boxplot_stats(x, whis=1.5) defines them; sorted_out (may be null) [batch][n][ncol],
// the ascending column.  A column holding a NaN: n, then NaN in every other slot and in its sorted column.
// Dynamic LDS: RD_BOX_LDS_HEAD + npow2 floats.
__global__ void __launch_bounds__(RD_DIST_THREADS)
k_box_stats(const float* __restrict__ x, int n, int npow2, int ncol, double* __restrict__ stats, float* __restrict__ sorted_out) {
  extern __shared__ double rd_dist_lds[];
  double* red = rd_dist_lds;
  int* flag = (int*)(red + RD_DIST_THREADS);
  float* xs = (float*)(flag + 2);
  const int t = threadIdx.x;
  const long bt = blockIdx.x / ncol, c = blockIdx.x % ncol;
  if (t == 0) *flag = 0;
  __syncthreads();
  rd_dist_load_sort(x + bt * n * ncol + c, ncol, n, npow2, xs, flag);
  const bool bad = *flag != 0;
  double s = 0.0;
  for (int i = t; i < n; i += RD_DIST_THREADS) s += (double)xs[i];
  s = rd_block_sum_f64(s, red);
  if (sorted_out) {
    float* dst = sorted_out + bt * n * ncol + c;
    for (int i = t; i < n; i += RD_DIST_THREADS) dst[(long)i * ncol] = bad ? __builtin_nanf("") : xs[i];
  }
  if (t == 0) {
#pragma clang fp contract(off)
    double* o = stats + (long)blockIdx.x * RD_DIST_NSTATS;
    const double dn = (double)n;
    o[0] = dn;
    if (bad) {
      for (int k = 1; k < RD_DIST_NSTATS; ++k) o[k] = __builtin_nan("");
    } else {
      const double q1 = rd_np_quantile(xs, n, 0.25), med = rd_np_quantile(xs, n, 0.5), q3 = rd_np_quantile(xs, n, 0.75);
      const double iqr = q3 - q1;
      const double loval = q1 - 1.5 * iqr, hival = q3 + 1.5 * iqr;
      const int k = rd_count_le(xs, n, hival);             // the largest datum <= hival is xs[k - 1]
      const double whishi = (k == 0 || (double)xs[k - 1] < q3) ? q3 : (double)xs[k - 1];
      const int l = rd_count_lt(xs, n, loval);             // the smallest datum >= loval is xs[l]
      const double whislo = (l == n || (double)xs[l] > q1) ? q1 : (double)xs[l];
      const double notch = 1.57 * iqr / sqrt(dn);
      o[1] = s / dn;
      o[2] = q1;
      o[3] = med;
      o[4] = q3;
      o[5] = iqr;
      o[6] = whislo;
      o[7] = whishi;
      o[8] = med - notch;
      o[9] = med + notch;
      o[10] = (double)rd_count_lt(xs, n, whislo);
      o[11] = (double)(n - rd_count_le(xs, n, whishi));
    }
  }
}

// the slot of one value among the ascending thresholds g[0 .. T): the first j with g[j] >= v (T: above the last), T + 1 for a NaN
__device__ __forceinline__ int rd_ecdf_slot(const float* g, int T, float v) {
  if (v != v) return T + 1;
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// a thread counts a run of values falling into the same slot in a register and adds it once (dry fields: long runs of zeros)
__device__ __forceinline__ void rd_ecdf_add(const float* g, int T, unsigned* h, float v, int& last, unsigned& cnt) {
  const int s = rd_ecdf_slot(g, T, v);
  if (s == last) {
    ++cnt;
  } else {
    if (cnt) atomicAdd(&h[last], cnt);
    last = s;
    cnt = 1;
  }
}

// hist [T + 2] (zeroed by the caller) += the slot counts of x[0 .. n).  Blocks of 256 threads, at most RD_ECDF_MAXBLOCKS of them (so
// a block's 32-bit LDS counts cannot wrap below n = 2^40); float4 loads over the 16-byte aligned middle of x, two in flight per
// thread; the first and last (< 4) values go through the first threads of the grid.  Dynamic LDS: T floats + (T + 2) counts.
__global__ void __launch_bounds__(RD_ECDF_THREADS)
k_ecdf_grid(const float* __restrict__ x, long n, const float* __restrict__ grid, int T, unsigned long long* __restrict__ hist) {
  extern __shared__ float rd_ecdf_lds[];
  float* g = rd_ecdf_lds;
  unsigned* h = (unsigned*)(g + T);
  const int t = threadIdx.x;
  for (int i = t; i < T; i += RD_ECDF_THREADS) g[i] = grid[i];
  for (int i = t; i < T + 2; i += RD_ECDF_THREADS) h[i] = 0u;
  __syncthreads();
  long head = (long)(((16 - ((unsigned long long)x & 15)) & 15) >> 2);
  if (head > n) head = n;
  const float4* xv = (const float4*)(x + head);
  const long nv = (n - head) >> 2;
  const long tail0 = head + 4 * nv;
  const long gt = (long)blockIdx.x * RD_ECDF_THREADS + t, stride = (long)gridDim.x * RD_ECDF_THREADS;
  int last = 0;
  unsigned cnt = 0;
  for (long i = gt; i < nv; i += 2 * stride) {
    const bool two = i + stride < nv;
    const float4 v0 = xv[i];
    const float4 v1 = two ? xv[i + stride] : v0;
    rd_ecdf_add(g, T, h, v0.x, last, cnt);
    rd_ecdf_add(g, T, h, v0.y, last, cnt);
    rd_ecdf_add(g, T, h, v0.z, last, cnt);
    rd_ecdf_add(g, T, h, v0.w, last, cnt);
    if (two) {
      rd_ecdf_add(g, T, h, v1.x, last, cnt);
      rd_ecdf_add(g, T, h, v1.y, last, cnt);
      rd_ecdf_add(g, T, h, v1.z, last, cnt);
      rd_ecdf_add(g, T, h, v1.w, last, cnt);
    }
  }
  if (gt < head) rd_ecdf_add(g, T, h, x[gt], last, cnt);
  if (gt < n - tail0) rd_ecdf_add(g, T, h, x[tail0 + gt], last, cnt);
  if (cnt) atomicAdd(&h[last], cnt);
  __syncthreads();
  for (int i = t; i < T + 2; i += RD_ECDF_THREADS)
    if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// One 1024-thread block: counts[j] = hist[0] + .. + hist[j] = #{x <= grid[j]} for j < T; counts[T] = hist[T], the values above the
// last threshold; counts[T + 1] = hist[T + 1], the NaNs.  Thread t owns a contiguous chunk; a scan of the chunk sums gives its offset.
__global__ void __launch_bounds__(RD_DIST_THREADS)
k_ecdf_scan(const unsigned long long* __restrict__ hist, int T, long long* __restrict__ counts) {
  __shared__ unsigned long long red[RD_DIST_THREADS];
  const int t = threadIdx.x;
  const int c = (T + RD_DIST_THREADS - 1) / RD_DIST_THREADS;
  const int i0 = min(t * c, T), i1 = min(i0 + c, T);
  unsigned long long s = 0;
  for (int i = i0; i < i1; ++i) s += hist[i];
  red[t] = s;
  __syncthreads();
  for (int off = 1; off < RD_DIST_THREADS; off <<= 1) {
    const unsigned long long v = t >= off ? red[t - off] : 0ull;
    __syncthreads();
    red[t] += v;
    __syncthreads();
  }
  unsigned long long run = t > 0 ? red[t - 1] : 0ull;
  for (int i = i0; i < i1; ++i) {
    run += hist[i];
    counts[i] = (long long)run;
  }
  if (t < 2) counts[T + t] = (long long)hist[T + t];
}
