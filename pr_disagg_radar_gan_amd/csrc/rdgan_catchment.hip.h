// Catchment rainfall of hourly fields: the areal rainfall of every basin of a map, hour by hour, its largest
// k-hour accumulation per day and statistics of those maxima over the days.
// hourly [n][24][ny][nx] fp32 with a leading stride day_stride >= 24 ny nx.  q = (int) rintf(x * 1024) in units of 2^-10 mm; a
// pixel-hour is bad when x is NaN, +-inf, negative or >= 2048: rd_depth_q and rd_depth_bad (so q < 2^21).  A catchment is a list of
// pixels: pixels[E] holds the flat indices y nx + x of all catchments one behind the other, and a pixel may stand in several lists
// (nested basins) or in none.  The kernels see the lists only through the chunk table chunks[n_chunks][3] = (catchment, first
// entry, count): a run of 1 .. RD_CT_CHUNK consecutive entries of ONE catchment.
// P[d][c][h] is the sum of q over the pixels of catchment c at hour h of day d (a bad pixel-hour adds 0), B[d][c][h] the number
// of its bad pixel-hours; an hour with B > 0 is void.  For a window k the day's key is the maximum over the start hours h0 whose k
// hours are all clean of (P[h0] + .. + P[h0 + k - 1]) 32 + (31 - h0): the largest sum A < 2^50, and among equal ones the
// smallest h0; never 0, so 0 means "no clean window".
//
// A pass holds D whole days in the workspace: P [D][C][24] int64, then B [D][C][24] int32, zeroed by the entry before the pass.
//  * k_catch_sums: the only read of the hourly array.  One workgroup per (chunk, day); a lane takes one list entry and walks the
//    24 hours (lists are in raster order, so the lanes of a wave mostly read runs of adjacent pixels).  The 24 sums are reduced
//    across the wave by a halving butterfly -- at each of the first three steps a lane hands one half of its values to its partner
//    and keeps the sums of the other half, 12 + 6 + 3 exchanges, then 3 values go through the last three steps: 30 exchanges
//    instead of 144 -- in 32 bits (64 q < 2^27), and from there on in 64 bits: across the waves in LDS, then one 64-bit atomic
//    add per hour and workgroup into P.  The bad pixel-hours are counted in LDS (rare, so the common path is a skipped branch) and
//    added to B only where there are any.
//  * k_catch_days: one thread per (day, catchment) of the pass.  It slides every window over the 24 hours of P and B, keeps the
//    largest key, classifies the day into the (c, k) record of the state with 64-bit integer atomics and writes series_out and
//    depths_out.  It clears nothing.
// Kernel boundaries are the only ordering between the phases: no spin-wait, no grid sync, no floating-point atomic.  All global
// offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_CT_THREADS 256
#define RD_CT_CHUNK 256                  // list entries of a chunk: one per lane of a workgroup
#define RD_CT_MAXK 8                     // windows
#define RD_CT_MAXL 16                    // levels
#define RD_CT_MAXCATCH 65535
#define RD_CT_MAXENTRIES (1L << 26)
#define RD_CT_MAXCHUNKS (1L << 19)       // above MAXENTRIES / CHUNK + MAXCATCH, what a table with no needless cut holds
#define RD_CT_MAXGROUPS ((1L << 24) - 1) // workgroups of a launch: fewer than 2^32 threads
#define RD_CT_MAXPASS 65535              // days of one pass: the grid's y
// the record of one (c, k), L levels: level_count[L + 1], then at L + 1 +
#define RD_CT_START 0                    // start_hour[24]
#define RD_CT_SUM_A 24
#define RD_CT_MAX_A 25
#define RD_CT_NDAYS 26
#define RD_CT_NVOID 27
#define RD_CT_NDRY 28
#define RD_CT_FIXED 29                   // words of a record besides level_count

struct rd_ct_lists {
  int K, L;                              // windows, levels
  int windows[RD_CT_MAXK];
  long long level_q[RD_CT_MAXL];         // rd_levels_q
};

__host__ __device__ inline long rd_ct_record(int L) { return L + 1 + RD_CT_FIXED; }
__host__ __device__ inline long rd_ct_state_count(long C, int K, int L) { return C * K * rd_ct_record(L) + 2; }
// bytes of the workspace per day: 24 sums of 8 bytes and 24 bad counts of 4 per catchment
__host__ __device__ inline long rd_ct_day_bytes(long C) { return C * RD_HOURS * 12; }

// One step of the halving butterfly over N values: the lanes with bit M clear keep the sums of v[0 .. N/2 - 1], their partners
// lane ^ M those of v[N/2 .. N - 1]; each hands the other half over.
template <int N, int M>
__device__ __forceinline__ void rd_ct_halve(unsigned (&v)[RD_HOURS], bool upper) {
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const unsigned keep = upper ? v[i + N / 2] : v[i], send = upper ? v[i] : v[i + N / 2];
    v[i] = keep + (unsigned)__shfl_xor((int)send, M);
  }
}

// grid (n_chunks, D).  P and B: the pass's sums, zeroed before the launch.
__global__ void __launch_bounds__(RD_CT_THREADS)
k_catch_sums(const float* __restrict__ hourly, long day_stride, long plane, long day0, const int* __restrict__ chunks,
             const int* __restrict__ pixels, long n_entries, int n_catch, unsigned long long* __restrict__ P, unsigned* __restrict__ B) {
  __shared__ unsigned long long sP[RD_HOURS];
  __shared__ unsigned sB[RD_HOURS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int* ch = chunks + (long)blockIdx.x * 3;
  const int c = ch[0], count = ch[2];
  const long first = ch[1];
  // (the table is checked on the host; a chunk that would leave the lists or the state is skipped whole)
  if (c < 0 || c >= n_catch || first < 0 || count < 1 || count > RD_CT_CHUNK || first + count > n_entries) return;
  if (tid < RD_HOURS) sP[tid] = 0ull, sB[tid] = 0u;
  __syncthreads();
  if (tid - lane < count) {                                                  // a wave with an entry
    unsigned v[RD_HOURS];
    const long p = tid < count ? (long)pixels[first + tid] : -1;
    if (p >= 0 && p < plane) {
      const float* xd = hourly + (day0 + (long)blockIdx.y) * day_stride + p;
      float f[RD_HOURS];
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) f[h] = xd[h * plane];
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) {
        const bool b = rd_depth_bad(f[h]);
        v[h] = b ? 0u : (unsigned)rd_depth_q(f[h]);
        if (b) atomicAdd(&sB[h], 1u);
      }
    } else {
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) v[h] = 0u;
    }
    rd_ct_halve<24, 32>(v, lane & 32);
    rd_ct_halve<12, 16>(v, lane & 16);
    rd_ct_halve<6, 8>(v, lane & 8);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int m = 4; m > 0; m >>= 1) v[i] += (unsigned)__shfl_xor((int)v[i], m);
    }
    if ((lane & 7) == 0) {                                                   // 8 lanes hold 3 hours each
      const int h = (lane & 32 ? 12 : 0) + (lane & 16 ? 6 : 0) + (lane & 8 ? 3 : 0);
#pragma unroll
      for (int i = 0; i < 3; ++i) atomicAdd(&sP[h + i], (unsigned long long)v[i]);
    }
  }
  __syncthreads();
  if (tid < RD_HOURS) {
    const long at = (((long)blockIdx.y * n_catch) + c) * RD_HOURS + tid;
    atomicAdd(&P[at], sP[tid]);
    if (sB[tid]) atomicAdd(&B[at], sB[tid]);
  }
}

// grid ceil(D C / 256); counts: the whole state; series and depths: null, or the maps of the whole input, day0 the first day of
// the pass
__global__ void __launch_bounds__(RD_CT_THREADS)
k_catch_days(int D, long day0, int n_catch, rd_ct_lists lists, const int* __restrict__ npix, const unsigned long long* __restrict__ P,
             const unsigned* __restrict__ B, unsigned long long* __restrict__ counts, long long* __restrict__ series,
             long long* __restrict__ depths) {
  const long t = (long)blockIdx.x * RD_CT_THREADS + threadIdx.x;            // day-major: the lanes of a wave take different records
  const int K = lists.K, L = lists.L;
  const long rec = rd_ct_record(L);
  unsigned long long* tail = counts + (long)n_catch * K * rec;              // n_days_total, n_bad
  if (t == 0) atomicAdd(&tail[0], (unsigned long long)D);
  if (t >= (long)D * n_catch) return;
  const int c = (int)(t % n_catch);
  const long d = t / n_catch;
  const unsigned long long* Pd = P + t * RD_HOURS;
  const unsigned* Bd = B + t * RD_HOURS;
  unsigned long long bad = 0ull;
  for (int h = 0; h < RD_HOURS; ++h) bad += Bd[h];
  if (bad) atomicAdd(&tail[1], bad);
  if (series) {
    long long* out = series + ((day0 + d) * n_catch + c) * RD_HOURS;
    for (int h = 0; h < RD_HOURS; ++h) out[h] = Bd[h] ? -1ll : (long long)Pd[h];
  }
  const unsigned long long area = (unsigned long long)npix[c];
  for (int ki = 0; ki < K; ++ki) {
    const int k = lists.windows[ki];
    unsigned long long sum = 0ull, best = 0ull;
    unsigned nb = 0u;
    for (int h = 0; h < RD_HOURS; ++h) {
      sum += Pd[h], nb += Bd[h];
      if (h >= k) sum -= Pd[h - k], nb -= Bd[h - k];
      if (h >= k - 1 && !nb) {
        const unsigned long long key = (sum << 5) + (unsigned long long)(31 - (h - k + 1));
        best = key > best ? key : best;
      }
    }
    unsigned long long* r = counts + ((long)c * K + ki) * rec;
    unsigned long long* fixed = r + L + 1;
    long long depth = -1;
    if (!best) {
      atomicAdd(&fixed[RD_CT_NVOID], 1ull);
    } else {
      const unsigned long long A = best >> 5;
      depth = (long long)A;
      int b = 0;
      for (int l = 0; l < L; ++l) b += A >= (unsigned long long)lists.level_q[l] * area;
      atomicAdd(&r[b], 1ull);
      atomicAdd(&fixed[RD_CT_NDAYS], 1ull);
      if (A) {
        atomicAdd(&fixed[RD_CT_START + 31 - (int)(best & 31)], 1ull);
        atomicAdd(&fixed[RD_CT_SUM_A], A);
        atomicMax(&fixed[RD_CT_MAX_A], A);
      } else {
        atomicAdd(&fixed[RD_CT_NDRY], 1ull);
      }
    }
    if (depths) depths[((day0 + d) * n_catch + c) * K + ki] = depth;
  }
}
