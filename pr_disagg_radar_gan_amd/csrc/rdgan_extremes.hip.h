// Extremes of hourly fields: the largest k-hour accumulation of every pixel over the days of a block (a year,
// or member * B + year), and the integer sums the L-moments of a series of such maxima are formed from.
//
//  * k_block_maxima: hourly [n][24][plane] fp32 with a leading stride day_stride >= 24 plane; block[n] ints, the block of every day,
//    each in 0 .. NB - 1 (the entry checks them on the host).  q = rd_depth_q(x); a pixel-day with an rd_depth_bad hour is void.  For
//    the windows of `mask` (bit w - 1: a window of w hours, K = popcount) the day's depth is the largest q[h0] + .. + q[h0 + w - 1]
//    over h0 = 0 .. 24 - w: windows lie within the day, none crosses midnight.  A sum is below 24 * 2^21 < 2^26: 32 bits hold it.
//      bmax [NB][K][plane] int64: the largest depth of any good day of the block, -1 where there is none (the caller's initial value)
//      ndays, nvoid [NB][plane] int32: the good and the void pixel-days
//    A thread owns V adjacent pixels (V = 4: one 16-byte load per hour, rd_vec4_ok on the flat plane) and a workgroup a run of
//    `run` consecutive days of its 256 V pixels.  The 24 hours are loaded into registers, quantised and turned into prefix sums
//    c[0 .. 24] in place; a window sum is c[h0 + w] - c[h0], every index a compile-time constant (no scratch).  The K running maxima
//    of the thread's pixels live in its own LDS slot m[k][thread] (k is a run-time count, so registers would need a dynamic
//    index), the two day counts in registers.  While the day's block stays the same nothing leaves the workgroup; when it changes,
//    and at the end of the run, the thread issues one 64-bit atomicMax per (window, pixel) that saw a good day and one 32-bit
//    atomicAdd per non-zero count.  Days of one block are usually adjacent, so a block of 45 days costs a few atomics per pixel
//    instead of 45 on one address.  A slot belongs to one thread: there is no barrier.
//  * k_lmoment_sums: table [S][B][M] int64, B <= 128: S series of B block maxima at M positions.  An entry below 0, or one whose
//    ndays entry (same shape, int32, optional) is below min_days, is left out.  Per (s, m), over the ascending order statistics
//    x_(1) <= .. <= x_(n) of the entries kept:
//      n;  A0 = sum x_(j);  A1 = sum (j - 1) x_(j);  A2 = sum (j - 1)(j - 2) x_(j)          (entries < 2^40: A2 < 2^40 128^3 = 2^61)
//    sums [S][M][3] int64, n_out [S][M] int32, sorted_out null or [S][B][M] int64: ascending, then -1 for every entry left out.
//    A workgroup takes a run of 64 adjacent positions of one series: the B x 64 tile sits in LDS as key[b][px], positions innermost
//    as in k_member_stats (rdgan_products.hip.h), so the global read is 512 contiguous bytes per row and the 64 lanes of a wave read
//    64 consecutive 8-byte words of one row in the rank loop, free of bank conflicts.  The key of an entry left out is the largest
//    int64.  The rank of entry b is the number of entries b' with key[b'] < key[b], or equal and b' < b: a permutation of 0 .. B - 1
//    that puts the kept entries first in ascending order.  A thread ranks four entries of its position at once (one LDS read serves
//    four compares), O(B^2 / 4) reads per position.  The sums are invariant under the order of tied values, so the index tie rule
//    shows in nothing but which of two equal values is written first.  Partial sums meet in LDS through 64-bit integer atomics.
// No floating-point atomics; every result is an integer that does not depend on the launch geometry.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_EX_THREADS 256
#define RD_EX_MAXK 8                     // windows (RD_PEAKS_MAXK)
#define RD_EX_MAXSTATE (1L << 31)        // NB K plane: entries of bmax, 16 GiB
#define RD_EX_MAXBLOCKS (1L << 31)       // NB
#define RD_EX_MAXRUN 4096                // days of a workgroup's run
#define RD_EX_MINRUN 8                   // ... where the entry chooses, at least these (fewer atomics per address)
#define RD_EX_MAXB 128                   // blocks of a series
#define RD_EX_PX 64                      // positions of a tile
#define RD_EX_MAXVALUE (1LL << 40)       // a maximum is below this
#define RD_EX_LDS_HEAD (3 * RD_EX_PX * sizeof(unsigned long long) + RD_EX_PX * sizeof(unsigned))
#define RD_EX_LDS_MAX (RD_EX_LDS_HEAD + (size_t)RD_EX_MAXB * RD_EX_PX * sizeof(long long))

// the largest sum of W consecutive hours from the prefix sums c[0 .. 24]
template <int W> __device__ __forceinline__ int rd_ex_window_max(const int (&c)[RD_HOURS + 1]) {
  int best = c[W] - c[0];
#pragma unroll
  for (int h0 = 1; h0 + W <= RD_HOURS; ++h0) best = max(best, c[h0 + W] - c[h0]);
  return best;
}

// what a thread has gathered for block b goes to the state: pixels p .. p + V - 1 (all inside the plane)
template <int V>
__device__ __forceinline__ void rd_ex_flush(long b, int K, long plane, long p, const int (*m)[RD_EX_THREADS * V], const int (&nd)[V],
                                            const int (&nv)[V], long long* __restrict__ bmax, int* __restrict__ ndays,
                                            int* __restrict__ nvoid) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (nd[j]) {
      atomicAdd(&ndays[b * plane + p + j], nd[j]);
      for (int k = 0; k < K; ++k) atomicMax(&bmax[(b * K + k) * plane + p + j], (long long)m[k][t * V + j]);
    }
    if (nv[j]) atomicAdd(&nvoid[b * plane + p + j], nv[j]);
  }
}

// grid groups * ceil(n / run), groups = ceil(plane / (256 V)): workgroup g + groups r takes pixel group g of run r
template <int V>
__global__ void __launch_bounds__(RD_EX_THREADS)
k_block_maxima(const float* __restrict__ hourly, long n, long day_stride, long plane, const int* __restrict__ block, long NB, unsigned mask,
               int run, long groups, long long* __restrict__ bmax, int* __restrict__ ndays, int* __restrict__ nvoid) {
  __shared__ int m[RD_EX_MAXK][RD_EX_THREADS * V];
  const int t = threadIdx.x;
  const long p = (((long)blockIdx.x % groups) * RD_EX_THREADS + t) * V;
  if (p >= plane) return;                                                    // (V = 4: plane % 4 == 0, so p + 3 < plane too)
  const int K = __popc(mask);
  const long d0 = ((long)blockIdx.x / groups) * run, d1 = min(n, d0 + run);
  long cur = -1;
  int nd[V], nv[V];
  for (long d = d0; d < d1; ++d) {
    const long b = block[d];
    if (b < 0 || b >= NB) continue;                                          // (checked on the host: never taken)
    if (b != cur) {
      if (cur >= 0) rd_ex_flush<V>(cur, K, plane, p, m, nd, nv, bmax, ndays, nvoid);
      cur = b;
#pragma unroll
      for (int j = 0; j < V; ++j) nd[j] = nv[j] = 0;
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int j = 0; j < V; ++j) m[k][t * V + j] = -1;
      }
    }
    const float* xd = hourly + d * day_stride + p;
    float f[RD_HOURS][V];
#pragma unroll
    for (int h = 0; h < RD_HOURS; ++h) rd_load<V>(xd + h * plane, f[h]);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      int c[RD_HOURS + 1];
      bool bad = false;
      c[0] = 0;
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) {
        const bool b = rd_depth_bad(f[h][j]);
        bad |= b;
        c[h + 1] = c[h] + (b ? 0 : rd_depth_q(f[h][j]));
      }
      nd[j] += !bad, nv[j] += bad;
      if (bad) continue;
      int k = 0;
#define RD_EX_WINDOW(W)                                               \
  if (mask & (1u << (W - 1))) {                                       \
    int* slot = &m[k++][t * V + j];                                   \
    *slot = max(*slot, rd_ex_window_max<W>(c));                       \
  }
      RD_EX_WINDOW(1) RD_EX_WINDOW(2) RD_EX_WINDOW(3) RD_EX_WINDOW(4) RD_EX_WINDOW(5) RD_EX_WINDOW(6) RD_EX_WINDOW(7) RD_EX_WINDOW(8)
      RD_EX_WINDOW(9) RD_EX_WINDOW(10) RD_EX_WINDOW(11) RD_EX_WINDOW(12) RD_EX_WINDOW(13) RD_EX_WINDOW(14) RD_EX_WINDOW(15)
      RD_EX_WINDOW(16) RD_EX_WINDOW(17) RD_EX_WINDOW(18) RD_EX_WINDOW(19) RD_EX_WINDOW(20) RD_EX_WINDOW(21) RD_EX_WINDOW(22)
      RD_EX_WINDOW(23) RD_EX_WINDOW(24)
#undef RD_EX_WINDOW
    }
  }
  if (cur >= 0) rd_ex_flush<V>(cur, K, plane, p, m, nd, nv, bmax, ndays, nvoid);
}

// grid: up to 2^20 workgroups over the S * ceil(M / 64) tiles; dynamic LDS RD_EX_LDS_HEAD + B * 64 * 8 bytes
__global__ void __launch_bounds__(RD_EX_THREADS)
k_lmoment_sums(const long long* __restrict__ table, const int* __restrict__ ndays, int min_days, long S, int B, long M,
               long long* __restrict__ sums, int* __restrict__ n_out, long long* __restrict__ sorted) {
  extern __shared__ unsigned long long rd_ex_lds[];
  unsigned long long* acc = rd_ex_lds;                                       // [3][PX]
  unsigned* cnt = (unsigned*)(acc + 3 * RD_EX_PX);                           // [PX]
  long long* key = (long long*)(rd_ex_lds + 3 * RD_EX_PX + RD_EX_PX / 2);    // [B][PX]
  const int t = threadIdx.x, px = t & (RD_EX_PX - 1), g = t / RD_EX_PX;
  constexpr int G = RD_EX_THREADS / RD_EX_PX;
  const long long kLeftOut = 0x7FFFFFFFFFFFFFFFLL;
  const long runs = (M + RD_EX_PX - 1) / RD_EX_PX, tiles = S * runs;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long s = tile / runs, pos = (tile % runs) * RD_EX_PX + px;
    const bool live = pos < M;
    __syncthreads();                                                         // the previous tile's outputs have been formed
    if (t < RD_EX_PX) acc[t] = acc[RD_EX_PX + t] = acc[2 * RD_EX_PX + t] = 0ull, cnt[t] = 0u;
    for (int b = g; b < B; b += G) {
      long long v = kLeftOut;
      if (live) {
        const long at = (s * B + b) * M + pos;
        const long long x = table[at];
        if (x >= 0 && !(ndays && ndays[at] < min_days)) v = x;
      }
      key[b * RD_EX_PX + px] = v;
    }
    __syncthreads();
    unsigned long long a0 = 0ull, a1 = 0ull, a2 = 0ull;
    unsigned kept = 0u;
    for (int b0 = g * 4; b0 < B; b0 += G * 4) {
      long long mine[4];
      int rank[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) mine[i] = b0 + i < B ? key[(b0 + i) * RD_EX_PX + px] : kLeftOut, rank[i] = 0;
      for (int o = 0; o < B; ++o) {
        const long long v = key[o * RD_EX_PX + px];
#pragma unroll
        for (int i = 0; i < 4; ++i) rank[i] += (v < mine[i]) | ((v == mine[i]) & (o < b0 + i));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (b0 + i >= B || !live) continue;
        const bool in = mine[i] != kLeftOut;
        if (in) {
          const unsigned long long x = (unsigned long long)mine[i], r = (unsigned long long)rank[i];   // r = j - 1
          a0 += x, a1 += r * x, a2 += r * (r - 1) * x;                       // (r = 0: r (r - 1) = 0 before it wraps)
          ++kept;
        }
        if (sorted) sorted[(s * B + rank[i]) * M + pos] = in ? mine[i] : -1ll;
      }
    }
    if (kept) {
      atomicAdd(&acc[px], a0), atomicAdd(&acc[RD_EX_PX + px], a1), atomicAdd(&acc[2 * RD_EX_PX + px], a2);
      atomicAdd(&cnt[px], kept);
    }
    __syncthreads();
    if (t < RD_EX_PX && live) {
      long long* out = sums + (s * M + pos) * 3;
      out[0] = (long long)acc[t], out[1] = (long long)acc[RD_EX_PX + t], out[2] = (long long)acc[2 * RD_EX_PX + t];
      n_out[s * M + pos] = (int)cnt[t];
    }
  }
}
