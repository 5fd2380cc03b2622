// Multivariate rank histograms: the pre-ranks of an observed hourly day among the members of an ensemble, after
// Thorarinsdottir, Scheuerer & Heinz (2016) -- average rank and band depth -- and Smith & Hansen / Wilks (2004) -- the minimum
// spanning tree.  Everything that leaves a kernel is an integer.
// A case is z_0 = the observation and z_1 .. z_m = the members, N = m + 1 vectors of 24 ny nx fp32 values.  A position is valid when
// all N values are finite there.  Per valid position p and per i, with comparisons in fp32 (so -0.0 == 0.0):
//   lt_i = #{j : z_j[p] < z_i[p]},  gt_i = #{j : z_j[p] > z_i[p]}
//   avg_i   += lt_i - gt_i + N + 1                                   (twice the mid-rank)
//   depth_i += (N - 1)(N - 2) - lt_i (lt_i - 1) - gt_i (gt_i - 1)    (twice the pairs of other vectors whose closed interval holds z_i[p])
// A column whose N values are all equal has lt = gt = 0: it adds N + 1 and (N - 1)(N - 2) to every i, and is counted, not ranked.
// Kernels.
//  * k_mvr_ranks<TP>: a workgroup of 256 threads owns one (day, hour) plane and a run of tiles of TP adjacent positions.  The N x TP
//    tile sits in LDS as tile[i][p], positions innermost; TP = 64 / 32 / 16 / 8 for N <= 512 / 1024 / 2048 / 4096 keeps it within 128 KB.
//    Thread t has column p = t % TP and the rows i = t / TP (mod 256 / TP).  While it stages its rows it compares each value with the
//    observation's and tests it for finiteness, and raises the column's `varies` and `bad` flags in LDS; after the barrier a bad
//    column is dropped and a constant one counted.  For the others a thread keeps RD_MVR_OWN of its own values in registers and walks
//    the column once: one LDS read of z_j[p] serves all of them, two compares and two adds each.  The two terms of a row are summed
//    over the tile's columns by xor shuffles among the TP lanes that share the row, and the lane of column 0 -- the only owner of
//    row i in the workgroup -- adds them to 64-bit sums in LDS, which leave at the end of the run as one 64-bit integer atomic per
//    (i, quantity).  Above RD_MVR_ACC_MAXN rows the 2 N sums do not fit beside the tile: there the row's terms leave after every
//    tile, and the end of the run adds only the constant columns' share.  The flags are kept twice, by the parity of the tile, so
//    that a tile costs two barriers.  sums [D][24][N][2] and n_valid [D][24] are zeroed before the launch.
//  * k_mvr_mst: dist [N][N] int64, symmetric, 0 <= entries < 2^40.  Workgroup i runs Prim's algorithm on the vertices other than i:
//    thread t keeps the keys of vertices t + 256 k, k < 16, in registers (no dynamic index: the loops over k are unrolled and the
//    in-tree flags are bits of one word); a step is the workgroup's smallest key << 12 | j -- xor shuffles in the wave, then the four
//    waves' minima through LDS, in two slots used in turn so that a step costs one barrier -- and one coalesced read of row j.  The
//    weights are integers, so the length does not depend on which of two equal edges is taken.  len [N] int64; N <= 2 gives 0.
// No floating-point atomics, no spin-wait, no grid sync; every result is independent of the launch geometry.  All global offsets are
// 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"
#include "rdgan_sequence.hip.h"          // RD_SEQ_MAXS

#define RD_MVR_THREADS 256
#define RD_MVR_MAXN RD_SEQ_MAXS          // vectors of a case: j takes 12 bits of an MST key
#define RD_MVR_MAXM (RD_MVR_MAXN - 1)    // members
#define RD_MVR_MAXDAYS (1L << 20)
#define RD_MVR_TILE_BYTES (128 * 1024)   // the N x TP fp32 tile
#define RD_MVR_MAXTP 64
#define RD_MVR_MINTP 8
#define RD_MVR_OWN 8                     // own values a thread ranks per LDS read
#define RD_MVR_ACC_MAXN 1024             // up to here the 2 N 64-bit sums of a run stay in LDS beside the tile
#define RD_MVR_TARGET_BLOCKS 2048        // workgroups a ranks launch aims at where the entry chooses the runs
#define RD_MVR_MAXDIST (1LL << 40)       // an MST edge is below this: key = length << 12 | j
#define RD_MVR_MST_KEYS (RD_MVR_MAXN / RD_MVR_THREADS)
#define RD_MVR_EMPTY (~0ull)

static_assert(RD_MVR_MAXN == 1 << 12 && RD_MVR_MAXN * RD_MVR_MINTP * 4 == RD_MVR_TILE_BYTES, "the widest case fits at the narrowest tile");
static_assert(RD_MVR_TILE_BYTES / 4L * RD_MVR_MAXN < (1L << 31), "a row's terms of one tile, at most TP (N - 1)(N - 2) with N TP values in the tile, are 32-bit");
static_assert(RD_MVR_THREADS == 256 && RD_MVR_MST_KEYS <= 32, "vertex j: thread j % 256, key j >> 8");

// positions of a tile: the widest of 64 / 32 / 16 / 8 at which N rows stay within RD_MVR_TILE_BYTES
__host__ __device__ inline int rd_mvr_tp(long n) {
  int tp = RD_MVR_MAXTP;
  while (tp > RD_MVR_MINTP && n * tp * 4 > RD_MVR_TILE_BYTES) tp >>= 1;
  return tp;
}
// dynamic LDS of k_mvr_ranks: the tile, then the sums of a run where they fit
__host__ __device__ inline long rd_mvr_lds_bytes(long n) { return n * rd_mvr_tp(n) * 4 + (n <= RD_MVR_ACC_MAXN ? n * 16 : 0); }

__device__ __forceinline__ bool rd_mvr_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// grid (D 24 runs): run fastest, then the (day, hour) plane.  ens_day_stride: m 24 P, or 0 for one ensemble shared by all days.
template <int TP>
__global__ void __launch_bounds__(RD_MVR_THREADS)
k_mvr_ranks(const float* __restrict__ ens, const float* __restrict__ obs, int N, long ens_day_stride, long P, long tiles, int runs,
            long tiles_per_run, unsigned long long* __restrict__ sums, unsigned long long* __restrict__ n_valid) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rd_mvr_lds[];
  __shared__ unsigned colbad[2][TP], colvar[2][TP], counts[2];
  float* tile = (float*)rd_mvr_lds;                                          // [N][TP]
  unsigned long long* acc = (unsigned long long*)(rd_mvr_lds + (size_t)N * TP * 4);   // [N][2] where acc_lds
  constexpr int G = RD_MVR_THREADS / TP;
  const bool acc_lds = N <= RD_MVR_ACC_MAXN;
  const int t = threadIdx.x, p = t % TP, g = t / TP;
  const int run = (int)(blockIdx.x % (unsigned)runs);
  const long dh = (long)(blockIdx.x / (unsigned)runs), d = dh / RD_HOURS, h = dh - d * RD_HOURS;
  const long member_stride = RD_HOURS * P;
  const float* op = obs + dh * P;
  const float* ep = ens + d * ens_day_stride + h * P;
  unsigned long long* out = sums + dh * N * 2;
  const int K1 = N + 1, K2 = (N - 1) * (N - 2);
  if (acc_lds)
    for (int i = t; i < 2 * N; i += RD_MVR_THREADS) acc[i] = 0ull;
  if (t < TP) colbad[0][t] = colbad[1][t] = colvar[0][t] = colvar[1][t] = 0u;
  if (t < 2) counts[t] = 0u;
  unsigned nv = 0u, nc = 0u;                                                 // (threads t < TP: the valid and the constant columns p of the run)
  const long tl0 = run * tiles_per_run, tl1 = min(tiles, tl0 + tiles_per_run);
  for (long tl = tl0; tl < tl1; ++tl) {
    const int par = (int)(tl & 1);
    const long pos = tl * TP + p;
    const bool in = pos < P;
    __syncthreads();                                                         // the previous tile has been ranked
    {
      const float ref = in ? op[pos] : 0.f;
      bool bad = !in || !rd_mvr_finite(ref), var = false;
#pragma unroll 4
      for (int i = g; i < N; i += G) {
        const float v = i == 0 || !in ? ref : ep[(long)(i - 1) * member_stride + pos];
        bad |= !rd_mvr_finite(v);
        var |= v != ref;
        tile[i * TP + p] = v;
      }
      if (bad) colbad[par][p] = 1u;
      if (var) colvar[par][p] = 1u;
    }
    __syncthreads();
    const bool valid = !colbad[par][p], active = valid && colvar[par][p];
    if (t < TP) {
      nv += valid, nc += valid && !active;
      colbad[par ^ 1][t] = colvar[par ^ 1][t] = 0u;                          // (last read a tile ago, next raised behind the barrier above)
    }
    if (!__any(active)) continue;                                            // (a dry hour: nothing to rank)
    for (int b0 = g; b0 < N; b0 += G * RD_MVR_OWN) {
      float mine[RD_MVR_OWN];
      int lt[RD_MVR_OWN], gt[RD_MVR_OWN];
#pragma unroll
      for (int r = 0; r < RD_MVR_OWN; ++r) {
        const int i = b0 + G * r;
        mine[r] = i < N ? tile[i * TP + p] : 0.f;
        lt[r] = gt[r] = 0;
      }
#pragma unroll 4
      for (int j = 0; j < N; ++j) {
        const float v = tile[j * TP + p];
#pragma unroll
        for (int r = 0; r < RD_MVR_OWN; ++r) lt[r] += v < mine[r], gt[r] += v > mine[r];
      }
#pragma unroll
      for (int r = 0; r < RD_MVR_OWN; ++r) {
        const int i = b0 + G * r;
        const bool on = active && i < N;
        int a = on ? lt[r] - gt[r] + K1 : 0, dp = on ? K2 - lt[r] * (lt[r] - 1) - gt[r] * (gt[r] - 1) : 0;
#pragma unroll
        for (int s = TP / 2; s > 0; s >>= 1) a += __shfl_xor(a, s), dp += __shfl_xor(dp, s);
        if (p == 0 && i < N && a) {                                          // (a > 0 as soon as one column of the tile is ranked)
          if (acc_lds) {
            acc[2 * i] += (unsigned long long)a, acc[2 * i + 1] += (unsigned long long)dp;
          } else {
            atomicAdd(&out[2 * i], (unsigned long long)a);
            if (dp) atomicAdd(&out[2 * i + 1], (unsigned long long)dp);
          }
        }
      }
    }
  }
  if (t < TP) {
    if (nv) atomicAdd(&counts[0], nv);
    if (nc) atomicAdd(&counts[1], nc);
  }
  __syncthreads();
  const unsigned long long nvt = counts[0], nct = counts[1];
  for (int i = t; i < N; i += RD_MVR_THREADS) {
    const unsigned long long a = (acc_lds ? acc[2 * i] : 0ull) + nct * (unsigned long long)K1;
    const unsigned long long dp = (acc_lds ? acc[2 * i + 1] : 0ull) + nct * (unsigned long long)K2;
    if (a) atomicAdd(&out[2 * i], a);
    if (dp) atomicAdd(&out[2 * i + 1], dp);
  }
  if (t == 0 && nvt) atomicAdd(&n_valid[dh], nvt);
}

// grid (N): workgroup i leaves vertex i out
__global__ void __launch_bounds__(RD_MVR_THREADS)
k_mvr_mst(const long long* __restrict__ dist, int N, long long* __restrict__ len) {
  __shared__ unsigned long long slot[2][RD_MVR_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, left = blockIdx.x;
  if (N <= 2) {                                                              // (uniform: at most one vertex is left)
    if (t == 0) len[left] = 0ll;
    return;
  }
  const int root = left == 0 ? 1 : 0;
  unsigned long long key[RD_MVR_MST_KEYS];
  unsigned open = 0u;                                                        // bit k: vertex t + 256 k is outside the tree and not left out
  {
    const long long* row = dist + (long)root * N;
#pragma unroll
    for (int k = 0; k < RD_MVR_MST_KEYS; ++k) {
      const int j = t + RD_MVR_THREADS * k;
      const bool in = j < N && j != left && j != root;
      key[k] = in ? (unsigned long long)row[j] : RD_MVR_EMPTY;
      open |= in ? 1u << k : 0u;
    }
  }
  unsigned long long total = 0ull;
  for (int step = 0; step < N - 2; ++step) {
    unsigned long long best = RD_MVR_EMPTY;
#pragma unroll
    for (int k = 0; k < RD_MVR_MST_KEYS; ++k) {
      const unsigned long long c = (key[k] << 12) | (unsigned long long)(t + RD_MVR_THREADS * k);
      if ((open >> k & 1u) && c < best) best = c;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const unsigned long long o = __shfl_xor(best, s);
      best = o < best ? o : best;
    }
    if (lane == 0) slot[step & 1][wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RD_MVR_THREADS / 64; ++w) {
      const unsigned long long o = slot[step & 1][w];
      best = o < best ? o : best;
    }
    const int u = (int)(best & 0xFFFull);
    if (best == RD_MVR_EMPTY || u >= N) break;                               // (uniform; only a matrix outside the precondition)
    total += best >> 12;
    if ((u & (RD_MVR_THREADS - 1)) == t) open &= ~(1u << (u >> 8));
    const long long* row = dist + (long)u * N;
#pragma unroll
    for (int k = 0; k < RD_MVR_MST_KEYS; ++k) {
      const int j = t + RD_MVR_THREADS * k;
      if (open >> k & 1u) {                                                  // (an open vertex lies below N)
        const unsigned long long dj = (unsigned long long)row[j];
        key[k] = dj < key[k] ? dj : key[k];
      }
    }
  }
  if (t == 0) len[left] = (long long)total;
}
