// Temporal structure of hourly fields: wet spells, transitions, wet hours per day, lagged products.
// x [n][24][plane] fp32 with a leading stride day_stride >= 24 plane; a series is the 24 hours of one (i, q), cut at the day
// boundary.  A series with a NaN or an inf adds 1 to n_bad and nothing else.  Hour h is wet for threshold t when x[h] > thr[t] in
// fp32; m is the 24-bit mask of wet hours.
//
//  * k_temporal_accumulate: one pass.  A thread owns V adjacent pixels (V = 4: 16-byte loads; V = 1: any 4-byte aligned view) and
//    holds their 24 hours in registers; the trip count of the grid-stride loop is the same in every lane, a lane past the end
//    carries zeros that count nowhere.
//    Counts, per threshold (a run-time loop over masks) in a per-workgroup LDS table of 32-bit words:
//      - the compare of hour h IS the wave's ballot of "hour h wet": wet[h] += popcount(B_h), t11[h] += popcount(B_h & B_h+1) are
//        scalar instructions, accumulated over the V pixels in scalar registers and added to LDS by one lane.  The four transition
//        counts of an hour pair are linear in (n_valid, wet[h], wet[h + 1], t11[h]) and are formed when the table is merged, so a
//        dry hour pair -- the hot bin trans[h][0][0] -- never touches LDS at all;
//      - wholly dry series are counted by ballot and popcount and one lane adds the sum to wet_hours[0], longest_wet[0] and
//        dry_spell[1][24]; only series with a wet hour issue LDS atomics of their own: popcount, first and last wet hour
//        (ctz / clz), and one atomic per run, the runs walked as pairs of set bits of m & ~(m << 1) and m & ~(m >> 1).
//    Sums, fp64, no atomics.  A thread forms the sum of a quantity over its V pixels; 16 (or 8) such quantities at a time are
//    written to a per-wave LDS tile [row][lane] and read back transposed, lane l adding the 16 (8) lanes of its segment for row
//    l % 16 in lane order: one LDS write, one LDS read and an add per quantity instead of a 6-step shuffle tree.  The lane adds that to an
//    accumulator it alone owns (registers for moments and lags, an LDS slot for wet_amount, whose index depends on the run-time
//    t).  At the end a thread per quantity adds the workgroup's accumulators in a fixed order and writes partial[block][quantity].
//    The table is merged into the state with 64-bit integer atomics (order-independent).
//    KMAX = 6 or 12 is the number of lags the instance forms (the smallest that covers K).
//  * k_temporal_final: one workgroup per quantity adds the workgroups' partials in a fixed order onto the state.
// Bounds: a workgroup handles fewer than 2^27 series (RD_TS_MAXBLOCKS workgroups, at most 2^40 elements per call), and a series
// adds at most 12 to one word, so no LDS word passes 2^31.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_TS_MAXT RD_THR_MAX
#define RD_TS_MAXK 12
#define RD_TS_THREADS 256
#define RD_TS_WAVES (RD_TS_THREADS / 64)
#define RD_TS_MAXBLOCKS 1024
// the state: counters per threshold, flat
#define RD_TS_WH 0                       // wet_hours[25]
#define RD_TS_LW 25                      // longest_wet[25]
#define RD_TS_WS 50                      // wet_spell[2][24]
#define RD_TS_DS 98                      // dry_spell[2][24]
#define RD_TS_FW 146                     // first_wet[24]
#define RD_TS_LAST 170                   // last_wet[24]
#define RD_TS_TR 194                     // trans[23][2][2]
#define RD_TS_NC 286
// the LDS table: the same up to trans, then wet[24] and t11[23] in its place
#define RD_TS_LWET 194
#define RD_TS_LT11 218
#define RD_TS_NL 242
#define RD_TS_LD 65                      // doubles per tile row: lanes 0 .. 63 and one of padding (conflict-free transposed reads)
#define RD_TS_TILE (16 * RD_TS_LD)       // doubles per wave

__host__ __device__ inline int rd_ts_nsums(int T, int K) { return 2 * RD_HOURS + K + T * RD_HOURS; }
__host__ __device__ inline size_t rd_ts_lds_bytes(int T) {
  return ((size_t)RD_TS_WAVES * RD_TS_TILE + (size_t)RD_TS_WAVES * T * 2 * 64) * sizeof(double) + ((size_t)T * RD_TS_NL + 2) * sizeof(unsigned);
}

// what one wave has written is visible to its own lanes: LDS operations of a wave complete in order, the fences keep the compiler
// from moving them
__device__ __forceinline__ void rd_ts_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the value, opaque to the compiler: a widening to fp64 is then formed where it is used and not kept for a later section (kept, the
// 96 doubles of a thread's four pixels are 192 registers)
__device__ __forceinline__ float rd_ts_again(float f) {
  asm volatile("" : "+v"(f));
  return f;
}

// R quantities of every lane -> this lane's sum, over the R lanes of segment lane / R in lane order, of quantity lane % R
template <int R, class F> __device__ __forceinline__ double rd_ts_fold(double* __restrict__ tile, int lane, F value) {
#pragma unroll
  for (int r = 0; r < R; ++r) tile[r * RD_TS_LD + lane] = value(r);
  rd_ts_wave_sync();
  const double* row = tile + (lane % R) * RD_TS_LD + (lane / R) * R;
  double s = row[0];
#pragma unroll
  for (int c = 1; c < R; ++c) s += row[c];
  rd_ts_wave_sync();
  return s;
}

// the runs of the set bits of r (24 bits): one count per run in bins[c][L - 1]; -> the longest
__device__ __forceinline__ int rd_ts_runs(unsigned* __restrict__ bins, unsigned r) {
  unsigned s = r & ~(r << 1), e = r & ~(r >> 1);
  int longest = 0;
  while (s) {
    const int a = __builtin_ctz(s), b = __builtin_ctz(e), L = b - a + 1;
    atomicAdd(&bins[((a == 0) | (b == RD_HOURS - 1)) * RD_HOURS + L - 1], 1u);
    longest = L > longest ? L : longest;
    s &= s - 1;
    e &= e - 1;
  }
  return longest;
}

template <int V, int KMAX>
__global__ void __launch_bounds__(RD_TS_THREADS)
k_temporal_accumulate(const float* __restrict__ x, long n, long day_stride, long plane, rd_thr thr, int T, int K,
                      unsigned long long* __restrict__ counts, double* __restrict__ partial) {
  extern __shared__ double rd_ts_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* tile = rd_ts_lds + wave * RD_TS_TILE;
  double* wacc = rd_ts_lds + RD_TS_WAVES * RD_TS_TILE + (long)wave * T * 2 * 64;          // [t][2][64], this wave's
  unsigned* tab = reinterpret_cast<unsigned*>(rd_ts_lds + RD_TS_WAVES * RD_TS_TILE + RD_TS_WAVES * T * 2 * 64);   // [T][NL], n_valid, n_bad
  for (int i = tid; i < RD_TS_WAVES * T * 2 * 64; i += RD_TS_THREADS) rd_ts_lds[RD_TS_WAVES * RD_TS_TILE + i] = 0.0;
  for (int i = tid; i < T * RD_TS_NL + 2; i += RD_TS_THREADS) tab[i] = 0u;
  __syncthreads();

  const long gpp = plane / V, groups = n * gpp;                          // (V = 4 is chosen only for plane % 4 == 0)
  double acc_m[3] = {0.0, 0.0, 0.0}, acc_l = 0.0;
  unsigned n_valid = 0, n_bad = 0;
  for (long g0 = (long)blockIdx.x * RD_TS_THREADS; g0 < groups; g0 += (long)gridDim.x * RD_TS_THREADS) {
    const long g = g0 + tid;
    const bool in = g < groups;
    float v[RD_HOURS][V];
    if (in) {
      const float* src = x + (g / gpp) * day_stride + (g % gpp) * V;
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) rd_load<V>(src + (long)h * plane, v[h]);
    } else {
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h)
#pragma unroll
        for (int j = 0; j < V; ++j) v[h][j] = 0.0f;
    }
    // a bad series is zeroed: it is never wet (thr >= 0) and adds +0.0 to every sum
    bool ok[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      unsigned worst = 0;
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) {
        const unsigned e = __float_as_uint(v[h][j]) & RD_F32_EXP;
        worst = e > worst ? e : worst;
      }
      const bool finite = worst != RD_F32_EXP;
      ok[j] = in && finite;
      n_valid += ok[j];
      n_bad += in && !finite;
      if (!finite) {
#pragma unroll
        for (int h = 0; h < RD_HOURS; ++h) v[h][j] = 0.0f;
      }
    }

    // moments: quantity 2 h is sum x[h], 2 h + 1 is sum x[h]^2; 16 quantities (8 hours) per fold
#pragma unroll
    for (int b = 0; b < 3; ++b)
      acc_m[b] += rd_ts_fold<16>(tile, lane, [&](int r) {
        const int h = 8 * b + (r >> 1);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const double d = (double)rd_ts_again(v[h][j]);
          s = (r & 1) ? __builtin_fma(d, d, s) : s + d;
        }
        return s;
      });

    // lags: quantity k - 1 is the sum over h of x[h] x[h + k]; all KMAX of them are formed, the first K are kept at the end
    {
      double lg[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) lg[k] = 0.0;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        double d[RD_HOURS];
#pragma unroll
        for (int h = 0; h < RD_HOURS; ++h) d[h] = (double)rd_ts_again(v[h][j]);
#pragma unroll
        for (int h = 1; h < RD_HOURS; ++h)                      // (hours outer: a widened hour is live for KMAX hours only)
#pragma unroll
          for (int k = 1; k <= KMAX; ++k)
            if (h - k >= 0) lg[k - 1] = __builtin_fma(d[h - k], d[h], lg[k - 1]);
      }
      acc_l += rd_ts_fold<16>(tile, lane, [&](int r) { return r < KMAX ? lg[r < KMAX ? r : 0] : 0.0; });
    }

    for (int t = 0; t < T; ++t) {
      float th = thr.v[0];
#pragma unroll
      for (int k = 1; k < RD_TS_MAXT; ++k) th = k == t ? thr.v[k] : th;
      unsigned* ct = tab + t * RD_TS_NL;
      unsigned wet[RD_HOURS], t11[RD_HOURS - 1], n_dry = 0;          // the same in every lane: scalar registers
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) wet[h] = 0;
#pragma unroll
      for (int h = 0; h < RD_HOURS - 1; ++h) t11[h] = 0;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        unsigned m = 0;
        unsigned long long prev = 0;
#pragma unroll
        for (int h = 0; h < RD_HOURS; ++h) {
          const bool w = v[h][j] > th;
          const unsigned long long b = __ballot(w);
          m |= (unsigned)w << h;
          wet[h] += (unsigned)__popcll(b);
          if (h) t11[h - 1] += (unsigned)__popcll(b & prev);
          prev = b;
        }
        n_dry += (unsigned)__popcll(__ballot(ok[j] && m == 0));
        if (m) {                                                          // (a bad series has m == 0)
          atomicAdd(&ct[RD_TS_WH + __builtin_popcount(m)], 1u);
          atomicAdd(&ct[RD_TS_FW + __builtin_ctz(m)], 1u);
          atomicAdd(&ct[RD_TS_LAST + 31 - __builtin_clz(m)], 1u);
          atomicAdd(&ct[RD_TS_LW + rd_ts_runs(ct + RD_TS_WS, m)], 1u);
          rd_ts_runs(ct + RD_TS_DS, ~m & 0xFFFFFFu);
        }
      }
      if (lane == 0) {
        if (n_dry) {
          atomicAdd(&ct[RD_TS_WH], n_dry);
          atomicAdd(&ct[RD_TS_LW], n_dry);
          atomicAdd(&ct[RD_TS_DS + RD_HOURS + RD_HOURS - 1], n_dry);
        }
#pragma unroll
        for (int h = 0; h < RD_HOURS; ++h)
          if (wet[h]) atomicAdd(&ct[RD_TS_LWET + h], wet[h]);
#pragma unroll
        for (int h = 0; h < RD_HOURS - 1; ++h)
          if (t11[h]) atomicAdd(&ct[RD_TS_LT11 + h], t11[h]);
      }
      // wet_amount[t][h]: hours 0 .. 15, then 16 .. 23, onto the LDS slots this lane owns
      wacc[(t * 2 + 0) * 64 + lane] += rd_ts_fold<16>(tile, lane, [&](int r) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) s += (double)rd_ts_again(v[r][j] > th ? v[r][j] : 0.0f);
        return s;
      });
      wacc[(t * 2 + 1) * 64 + lane] += rd_ts_fold<8>(tile, lane, [&](int r) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) s += (double)rd_ts_again(v[16 + r][j] > th ? v[16 + r][j] : 0.0f);
        return s;
      });
    }
  }

  // the workgroup's accumulators, added in a fixed order: waves outer, segments inner
  if (n_valid) atomicAdd(&tab[T * RD_TS_NL], n_valid);
  if (n_bad) atomicAdd(&tab[T * RD_TS_NL + 1], n_bad);
  double* fin = rd_ts_lds;                                               // [4][256] over the tiles, which are free now
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 3; ++b) fin[b * RD_TS_THREADS + tid] = acc_m[b];
  fin[3 * RD_TS_THREADS + tid] = acc_l;
  __syncthreads();
  const int nsums = rd_ts_nsums(T, K);
  const double* wall = rd_ts_lds + RD_TS_WAVES * RD_TS_TILE;             // [wave][t][2][64]
  for (int i = tid; i < nsums; i += RD_TS_THREADS) {
    double s = 0.0;
    if (i < 2 * RD_HOURS + K) {
      const int b = i < 2 * RD_HOURS ? i >> 4 : 3, r = i < 2 * RD_HOURS ? i & 15 : i - 2 * RD_HOURS;
      for (int w = 0; w < RD_TS_WAVES; ++w)
        for (int sg = 0; sg < 4; ++sg) s += fin[b * RD_TS_THREADS + w * 64 + sg * 16 + r];
    } else {
      const int t = (i - 2 * RD_HOURS - K) / RD_HOURS, h = (i - 2 * RD_HOURS - K) % RD_HOURS;
      for (int w = 0; w < RD_TS_WAVES; ++w) {
        const double* a = wall + ((long)(w * T + t) * 2 + (h >= 16)) * 64;
        if (h < 16)
          for (int sg = 0; sg < 4; ++sg) s += a[sg * 16 + h];
        else
          for (int sg = 0; sg < 8; ++sg) s += a[sg * 8 + h - 16];
      }
    }
    partial[(long)blockIdx.x * nsums + i] = s;
  }
  // the table into the state
  const unsigned long long nv = tab[T * RD_TS_NL];
  for (int i = tid; i < T * RD_TS_TR; i += RD_TS_THREADS) {
    const int t = i / RD_TS_TR, c = i % RD_TS_TR;
    const unsigned val = tab[t * RD_TS_NL + c];
    if (val) atomicAdd(&counts[(long)t * RD_TS_NC + c], (unsigned long long)val);
  }
  for (int i = tid; i < T * (RD_HOURS - 1); i += RD_TS_THREADS) {
    const int t = i / (RD_HOURS - 1), h = i % (RD_HOURS - 1);
    const unsigned* ct = tab + t * RD_TS_NL;
    const unsigned long long w0 = ct[RD_TS_LWET + h], w1 = ct[RD_TS_LWET + h + 1], b = ct[RD_TS_LT11 + h];
    unsigned long long* dst = counts + (long)t * RD_TS_NC + RD_TS_TR + h * 4;
    if (nv + b - w0 - w1) atomicAdd(dst + 0, nv + b - w0 - w1);
    if (w1 - b) atomicAdd(dst + 1, w1 - b);
    if (w0 - b) atomicAdd(dst + 2, w0 - b);
    if (b) atomicAdd(dst + 3, b);
  }
  if (tid == 0) {
    if (nv) atomicAdd(&counts[(long)T * RD_TS_NC], nv);
    if (tab[T * RD_TS_NL + 1]) atomicAdd(&counts[(long)T * RD_TS_NC + 1], (unsigned long long)tab[T * RD_TS_NL + 1]);
  }
}

// one workgroup per quantity: thread i adds partials i, i + 256, .. in order, a fixed tree adds the threads, onto sums
__global__ void __launch_bounds__(RD_TS_THREADS)
k_temporal_final(const double* __restrict__ partial, int nblk, int nsums, double* __restrict__ sums) {
  __shared__ double red[RD_TS_THREADS];
  const int tid = threadIdx.x, q = blockIdx.x;
  double s = 0.0;
  for (int b = tid; b < nblk; b += RD_TS_THREADS) s += partial[(long)b * nsums + q];
  red[tid] = s;
  __syncthreads();
  for (int h = RD_TS_THREADS >> 1; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) sums[q] += red[0];
}
