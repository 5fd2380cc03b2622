// Least-cost assignment of the members of neighbouring days: for every boundary b of costs [B][S][S] int64
// with 0 <= C < 2^40 a permutation perm[b] that minimises sum_i C[b][i][perm[b][i]], and duals u[b], v[b] with
// u[i] + v[j] <= C[i][j] for all pairs and equality on the matched ones, which prove it.
// The algorithm is the definition (tests/assign_np.py restates it; perm, u and v agree bit for bit): shortest augmenting paths with
// dual potentials, the Hungarian method in Jonker-Volgenant form.  u = v = 0, no row matched.  Rows are inserted in the order
// 0 .. S - 1.  The insertion of row r is a Dijkstra search over the columns from a virtual column S with p[S] = r (p: column -> row):
//   minv[j] = inf, every column unused, j0 = S; then at most r + 1 steps:
//     i0 = p[j0]; for every unused j: cur = C[i0][j] - u[i0] - v[j]; if cur < minv[j] then minv[j] = cur, way[j] = j0;
//     (delta, j1) = the smallest (minv[j], j) over the unused j -- value first, then the smaller index;
//     u[p[j]] += delta and v[j] -= delta for every used j (the virtual one included: u[r] += delta), minv[j] -= delta for the others;
//     j0 = j1, now used; the search ends when p[j0] is free;
//   then the matching is flipped along way from j0 back to the virtual column: p[j0] = p[way[j0]], at most S hops.
// Range: an insertion raises the duals by less than 2^40 in all (the direct edge from r to a free column, whose v is 0, costs
// C < 2^40 in reduced terms and bounds the shortest path), so |u|, |v| < S 2^40 <= 2^52 and 0 <= minv < 2^52 at every step: plain
// int64, no scaling, and key = minv << 12 | j fits 64 bits.
//
// k_seq_assign: one workgroup of 256 threads per boundary holds the whole solve.  Thread t owns the columns t + 256 k, k = 0 .. 15,
// statically unrolled: their v and minv live in registers, the used flags in a bit mask.  What is indexed by data lies in LDS:
// u [S] by row, p [S + 1], way [S] (16 bits: a column or S).  A step reads p[j0] and u[i0] (broadcasts), loads the thread's unused
// columns of row i0 (8 bytes a lane, consecutive lanes consecutive: a row's start is 16-byte aligned only for even S), relaxes,
// reduces the keys by shuffles within a wave and one LDS round across the four waves (two slots by step parity, so a step has ONE
// barrier), and updates the duals.  u[p[j]] is touched only by the owner of the used column j, and the row a step reads, p[j1] of
// the column used last, has not been touched in this insertion: no barrier is needed for u inside a search.  Thread 0 flips the
// path between two barriers.  Every loop is a counted for; which column wins never depends on the launch geometry, since the keys
// of a boundary are distinct.  j1 = key & 4095 is the index of an unused column below S whatever the costs hold, and p holds rows
// or -1, so every global and LDS index is in range even outside the precondition.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_sequence.hip.h"

#define RD_ASG_THREADS 256
#define RD_ASG_COLS (RD_SEQ_MAXS / RD_ASG_THREADS)   // columns of a thread
#define RD_ASG_KEYBITS 12                            // key = minv << 12 | j
#define RD_ASG_INF (1ll << 62)

// |u|, |v| and minv stay below S 2^40 <= 2^52 (above), so minv << 12 does not leave 64 bits and a column index takes the rest
static_assert(RD_SEQ_MAXS == 1 << RD_ASG_KEYBITS && ((long)RD_SEQ_MAXS << 40) <= (1L << (64 - RD_ASG_KEYBITS)), "key = minv << 12 | j");
static_assert(RD_ASG_COLS * RD_ASG_THREADS == RD_SEQ_MAXS && RD_ASG_COLS <= 32, "a thread's used flags are one 32-bit mask");

// grid (B)
__global__ void __launch_bounds__(RD_ASG_THREADS)
k_seq_assign(const long long* __restrict__ costs, int S, int* __restrict__ perm, long long* __restrict__ u_out, long long* __restrict__ v_out,
             long long* __restrict__ total_out) {
  __shared__ long long u[RD_SEQ_MAXS];
  __shared__ int p[RD_SEQ_MAXS + 1];
  __shared__ unsigned short way[RD_SEQ_MAXS];
  __shared__ unsigned long long part[2][RD_ASG_THREADS / 64];
  __shared__ long long tot[RD_ASG_THREADS / 64];
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const long long* C = costs + b * S * S;
  long long v[RD_ASG_COLS], minv[RD_ASG_COLS];
  unsigned live = 0u;                                                      // the slots of this thread that are columns
#pragma unroll
  for (int k = 0; k < RD_ASG_COLS; ++k) {
    v[k] = 0;
    if (tid + RD_ASG_THREADS * k < S) live |= 1u << k;
  }
  for (int j = tid; j <= S; j += RD_ASG_THREADS) p[j] = -1;
  for (int i = tid; i < S; i += RD_ASG_THREADS) u[i] = 0;
  int flip = 0;
  for (int r = 0; r < S; ++r) {
#pragma unroll
    for (int k = 0; k < RD_ASG_COLS; ++k) minv[k] = RD_ASG_INF;
    unsigned used = 0u;
    if (tid == 0) p[S] = r;
    __syncthreads();                                                       // p as the last insertion left it, and p[S]
    int j0 = S;
    for (int step = 0; step <= r; ++step) {                                // (r columns are matched: a free one is met by then)
      const int i0 = p[j0];
      const long long ui = u[i0];
      const long long* row = C + (long)i0 * S;
      const unsigned open = live & ~used;
      long long c[RD_ASG_COLS];
#pragma unroll
      for (int k = 0; k < RD_ASG_COLS; ++k)
        if (open >> k & 1u) c[k] = row[tid + RD_ASG_THREADS * k];
      unsigned long long best = RD_SEQ_EMPTY;
#pragma unroll
      for (int k = 0; k < RD_ASG_COLS; ++k)
        if (open >> k & 1u) {
          const int j = tid + RD_ASG_THREADS * k;
          const long long cur = c[k] - ui - v[k];
          if (cur < minv[k]) minv[k] = cur, way[j] = (unsigned short)j0;
          const unsigned long long key = ((unsigned long long)minv[k] << RD_ASG_KEYBITS) | (unsigned long long)j;
          best = key < best ? key : best;
        }
      for (int sft = 32; sft > 0; sft >>= 1) {
        const unsigned long long o = __shfl_xor(best, sft);
        best = o < best ? o : best;
      }
      if ((tid & 63) == 0) part[flip][tid >> 6] = best;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < RD_ASG_THREADS / 64; ++w) best = part[flip][w] < best ? part[flip][w] : best;
      flip ^= 1;
      const long long delta = (long long)(best >> RD_ASG_KEYBITS);
      const int j1 = (int)(best & (RD_SEQ_MAXS - 1));
#pragma unroll
      for (int k = 0; k < RD_ASG_COLS; ++k)
        if (live >> k & 1u) {
          if (used >> k & 1u) u[p[tid + RD_ASG_THREADS * k]] += delta, v[k] -= delta;
          else minv[k] -= delta;
        }
      if (tid == 0) u[r] += delta;                                         // the virtual column
      j0 = j1;
      if ((j0 & (RD_ASG_THREADS - 1)) == tid) used |= 1u << (j0 / RD_ASG_THREADS);
      if (p[j0] < 0) break;                                                // (uniform)
    }
    __syncthreads();                                                       // way and u are complete, p has been read
    if (tid == 0)
      for (int hop = 0; hop < S; ++hop) {
        const int j1 = way[j0];
        p[j0] = p[j1];
        j0 = j1;
        if (j0 == S) break;
      }
  }
  __syncthreads();
  long long t = 0;
#pragma unroll
  for (int k = 0; k < RD_ASG_COLS; ++k)
    if (live >> k & 1u) {
      const int j = tid + RD_ASG_THREADS * k, i = p[j];
      perm[b * S + i] = j;
      v_out[b * S + j] = v[k];
      t += C[(long)i * S + j];
    }
  for (int i = tid; i < S; i += RD_ASG_THREADS) u_out[b * S + i] = u[i];
  for (int sft = 32; sft > 0; sft >>= 1) t += __shfl_xor(t, sft);
  if ((tid & 63) == 0) tot[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) total_out[b] = tot[0] + tot[1] + tot[2] + tot[3];
}
