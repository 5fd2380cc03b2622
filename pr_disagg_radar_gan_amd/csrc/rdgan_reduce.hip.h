// Scenario reduction: k representative members of an ensemble of hourly days by fast forward selection
// (Heitsch & Roemisch 2003, Algorithm 2.4) under the L1 distance of integer features, and the weight of each.
// Everything is an integer.  A member is [n_days][24][ny][nx] fp32.  A value is bad by rd_depth_bad; a good value has
// e = min(rint(x * 32), 65535) (rd_seq_feature).  With pool = p in {1, 2, 4, 8} a feature position is a p x p block of one plane,
// by = ceil(ny / p) rows of bx = ceil(nx / p) blocks, a rim block with its own pixel count n; its feature is (sum e + n / 2) / n in
// integer division, and it is bad when any of its pixels is.  Pf = n_days 24 by bx positions per member, padded to Ppad = 8 ceil(Pf / 8)
// with zeros that are never bad; a uint4 holds 8 positions, U = Ppad / 8.  A position is masked when it is bad in any member: the bad
// bits are ORed into one set of words [W], W = ceil(Ppad / 32), bit f % 32 of word f / 32, and applied when distances are formed.
// Dist[i][j] = sum over the unmasked positions of |e_i - e_j|, int64, symmetric, zero diagonal.
// Selection: m[j] = +inf; step t takes the unselected u with the smallest key = z[u] << 12 | u, z[u] = sum over j of min(m[j], Dist[u][j]),
// then m[j] = min(m[j], Dist[u][j]).  Assignment: assign[j] = the chosen u with the smallest Dist[u][j] << 12 | u.
// Kernels.
//  * k_red_features<VEC>: a thread owns 8 positions of one member, reads their p x p pixels (VEC: pool 1, two 16-byte loads), writes one
//    uint4 and ORs its bad bits into the words.
//  * k_red_valid: n_valid = Pf - popcount(bad), blocks meeting in a zeroed 64-bit counter.
//  * k_red_distances: k_seq_costs with both sides the same ensemble.  A workgroup of 256 threads owns a 64 x 64 tile of pairs (ti <= tj,
//    a linear index over the triangle) and a range of 128-position chunks; both panels staged in LDS as [uint4 of the chunk][member],
//    masked positions zeroed while staged, the next chunk fetched to registers meanwhile; a diagonal tile stages one panel and reads
//    it as both.  16 32-bit sums a thread, one v_sad_u16 per two positions of a pair, added to 64-bit sums every RD_SEQ_FLUSH chunks;
//    the ranges meet through 64-bit integer atomics in the zeroed matrix.  An off-diagonal tile adds each sum to [i][j] and [j][i]; a
//    diagonal tile holds both orders of a pair already and adds each to its own place, so nothing is added twice.
//  * k_red_select: a workgroup copies m to LDS; a wave owns a candidate row, its lanes stride over j, the sums meet by xor shuffles
//    and lane 0 lowers slot[t] (emptied to ~0 before the first step) by a 64-bit atomic minimum of the key.  Selected rows are skipped.
//  * k_red_update: reads slot[t]; writes chosen[t], cost[t], the selected flag and the new m.
//  * k_red_assign: a thread per member j walks the chosen list; counts[t] by an integer atomic add.
// Kernel boundaries are the only ordering: no spin-wait, no grid sync.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_sequence.hip.h"          // rd_seq_feature, rd_seq_keep2, the tile constants

#define RD_RED_MAXS RD_SEQ_MAXS          // members: u takes 12 bits of a key
#define RD_RED_MAXPOOL 8
#define RD_RED_KEYBITS 52                // z < 2^52: key = z << 12 | u fits 64 bits
#define RD_RED_ROWS 8                    // candidate rows of a workgroup of k_red_select: two a wave
#define RD_RED_TARGET_BLOCKS 2048        // workgroups a distances launch aims at
#define RD_RED_EMPTY (~0ull)

static_assert(RD_RED_MAXS == 1 << (64 - RD_RED_KEYBITS), "key = z << 12 | u");

__host__ __device__ inline long rd_red_blocks(long n, long pool) { return (n + pool - 1) / pool; }
__host__ __device__ inline long rd_red_tri(long tiles) { return tiles * (tiles + 1) / 2; }
// the workspace of a selection, bytes: m [S] and slot [k], 64-bit, then the selected flags
__host__ __device__ inline long rd_red_select_bytes(long s, long k) { return 8 * s + 8 * k + (s + 7) / 8 * 8; }

// the pooled feature of position f of a member (xp: its first value) and whether it is bad
__device__ __forceinline__ unsigned rd_red_pooled(const float* __restrict__ xp, long f, int ny, int nx, int pool, int by, int bx, bool& bad) {
  if (pool == 1) {
    const float v = xp[f];
    bad = rd_depth_bad(v);
    return bad ? 0u : rd_seq_feature(v);
  }
  const long per_plane = (long)by * bx, plane = f / per_plane;
  const int r = (int)(f - plane * per_plane), yb = r / bx, xb = r - yb * bx;
  const int y0 = yb * pool, x0 = xb * pool, y1 = min(y0 + pool, ny), x1 = min(x0 + pool, nx);
  const float* pp = xp + plane * ((long)ny * nx);
  unsigned sum = 0u;
  bool any = false;
  for (int y = y0; y < y1; ++y)
    for (int xx = x0; xx < x1; ++xx) {
      const float v = pp[(long)y * nx + xx];
      const bool b = rd_depth_bad(v);
      any |= b;
      sum += b ? 0u : rd_seq_feature(v);
    }
  bad = any;
  const unsigned n = (unsigned)((y1 - y0) * (x1 - x0));
  return any ? 0u : (sum + n / 2u) / n;
}

// grid (ceil(n_members U / 256)); item = member * U + c.  VEC: pool 1, x 16-byte aligned and member_stride a multiple of 4 (a member's
// 24 ny nx values are one already).  feat_stride in uint4.
template <bool VEC>
__global__ void __launch_bounds__(256)
k_red_features(const float* __restrict__ x, long n_members, long member_stride, long n_positions, int ny, int nx, int pool, int by, int bx,
               long U, uint4* __restrict__ feat, long feat_stride, unsigned* __restrict__ bad) {
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= n_members * U) return;
  const long member = item / U, c = item - member * U, f0 = c * 8;
  const float* xp = x + member * member_stride;
  unsigned e[8], bits = 0u;
  if constexpr (VEC) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (f0 < n_positions) a = *reinterpret_cast<const float4*>(xp + f0);
    if (f0 + 4 < n_positions) b = *reinterpret_cast<const float4*>(xp + f0 + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool bd = rd_depth_bad(v[i]);
      e[i] = bd ? 0u : rd_seq_feature(v[i]);
      bits |= bd ? 1u << i : 0u;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bool bd = false;
      e[i] = f0 + i < n_positions ? rd_red_pooled(xp, f0 + i, ny, nx, pool, by, bx, bd) : 0u;
      bits |= bd ? 1u << i : 0u;
    }
  }
  feat[member * feat_stride + c] = make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16);
  if (bits) atomicOr(&bad[c >> 2], bits << ((int)(c & 3) * 8));
}

// grid (ceil(W / 256), at most 1024): n_valid, zeroed before the launch, = n_positions - popcount(bad)
__global__ void __launch_bounds__(256)
k_red_valid(const unsigned* __restrict__ bad, long W, long n_positions, unsigned long long* __restrict__ n_valid) {
  unsigned long long count = 0ull;
  for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < W; w += (long)gridDim.x * 256) count += (unsigned long long)__popc(bad[w]);
  for (int s = 32; s > 0; s >>= 1) count += __shfl_xor(count, s);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long v = 0ull - count;                                   // (two's complement: the adds meet modulo 2^64)
    if (blockIdx.x == 0 && threadIdx.x == 0) v += (unsigned long long)n_positions;
    if (v) atomicAdd(n_valid, v);
  }
}

// grid (T (T + 1) / 2 * nsplit): split fastest, then the tile of the triangle, row tile by row tile.  stride: uint4 of a member.
// dist is zeroed before the launch.
__global__ void __launch_bounds__(RD_SEQ_THREADS)
k_red_distances(const uint4* __restrict__ feat, const unsigned* __restrict__ bad, int S, long stride, long U, int T, int nsplit,
                long chunks_per_split, unsigned long long* __restrict__ dist) {
  __shared__ __attribute__((aligned(16))) uint4 rows[RD_SEQ_CHUNK * RD_SEQ_LDU], cols[RD_SEQ_CHUNK * RD_SEQ_LDU];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int sp = (int)(blockIdx.x % (unsigned)nsplit);
  int rem = (int)(blockIdx.x / (unsigned)nsplit), ti = 0;
  while (rem >= T - ti) rem -= T - ti, ++ti;                               // (uniform; at most T = 64 steps)
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const long nchunks = (U + RD_SEQ_CHUNK - 1) / RD_SEQ_CHUNK;
  const long c0 = sp * chunks_per_split, c1 = min(c0 + chunks_per_split, nchunks);
  if (c0 >= c1) return;                                                    // (uniform)
  // the staging slots of this thread: q = 0 .. 3: member sm + 16 q of the tile, uint4 su of the chunk
  const int su = tid & (RD_SEQ_CHUNK - 1), sm = tid >> 4;
  rd_seq_stage st;
  auto fetch = [&](long c) {
    const long u = c * RD_SEQ_CHUNK + su;
    const bool in = u < U;
    const unsigned w = in ? bad[u >> 2] : 0u;
    st.bits = (w >> ((int)(u & 3) * 8)) & 0xFFu;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ma = ti * RD_SEQ_TILE + sm + 16 * q, mb = tj * RD_SEQ_TILE + sm + 16 * q;
      st.a[q] = in && ma < S ? feat[ma * stride + u] : make_uint4(0u, 0u, 0u, 0u);
      st.b[q] = !diag && in && mb < S ? feat[mb * stride + u] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  const uint4* colp = diag ? rows : cols;                                  // a diagonal tile stages once
  unsigned acc[4][4];
  unsigned long long tot[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = 0u, tot[r][k] = 0ull;
  fetch(c0);
  for (long c = c0; c < c1; ++c) {
    __syncthreads();                                                       // the previous chunk has been used
    {
      const unsigned k0 = rd_seq_keep2(st.bits, 0), k1 = rd_seq_keep2(st.bits, 1), k2 = rd_seq_keep2(st.bits, 2), k3 = rd_seq_keep2(st.bits, 3);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int at = su * RD_SEQ_LDU + sm + 16 * q;
        rows[at] = make_uint4(st.a[q].x & k0, st.a[q].y & k1, st.a[q].z & k2, st.a[q].w & k3);
        if (!diag) cols[at] = make_uint4(st.b[q].x & k0, st.b[q].y & k1, st.b[q].z & k2, st.b[q].w & k3);
      }
    }
    __syncthreads();
    if (c + 1 < c1) fetch(c + 1);
#pragma unroll 4
    for (int u = 0; u < RD_SEQ_CHUNK; ++u) {
      uint4 e[4], f[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = rows[u * RD_SEQ_LDU + ty + 16 * r];
#pragma unroll
      for (int k = 0; k < 4; ++k) f[k] = colp[u * RD_SEQ_LDU + tx + 16 * k];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          unsigned a = acc[r][k];
          a = __builtin_amdgcn_sad_u16(e[r].x, f[k].x, a);
          a = __builtin_amdgcn_sad_u16(e[r].y, f[k].y, a);
          a = __builtin_amdgcn_sad_u16(e[r].z, f[k].z, a);
          a = __builtin_amdgcn_sad_u16(e[r].w, f[k].w, a);
          acc[r][k] = a;
        }
    }
    if ((c - c0) % RD_SEQ_FLUSH == RD_SEQ_FLUSH - 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[r][k] += acc[r][k], acc[r][k] = 0u;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = ti * RD_SEQ_TILE + ty + 16 * r, j = tj * RD_SEQ_TILE + tx + 16 * k;
      const unsigned long long v = tot[r][k] + acc[r][k];
      if (i < S && j < S && v) {
        atomicAdd(&dist[(long)i * S + j], v);
        if (!diag) atomicAdd(&dist[(long)j * S + i], v);                   // (a diagonal tile has (j, i) among its own pairs)
      }
    }
}

// grid (ceil(S / RD_RED_ROWS)): slot -> slot[t]
__global__ void __launch_bounds__(256)
k_red_select(const long long* __restrict__ dist, int S, const unsigned long long* __restrict__ m, const unsigned char* __restrict__ selected,
             unsigned long long* __restrict__ slot) {
  __shared__ unsigned long long sm[RD_RED_MAXS];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int j = tid; j < S; j += 256) sm[j] = m[j];
  __syncthreads();
  for (int r = tid >> 6; r < RD_RED_ROWS; r += 4) {
    const int u = blockIdx.x * RD_RED_ROWS + r;
    if (u >= S || selected[u]) continue;                                   // (uniform in the wave)
    const long long* row = dist + (long)u * S;
    unsigned long long z = 0ull;
    for (int j = lane; j < S; j += 64) {
      const unsigned long long d = (unsigned long long)row[j];
      z += d < sm[j] ? d : sm[j];
    }
    for (int s = 32; s > 0; s >>= 1) z += __shfl_xor(z, s);
    if (lane == 0) atomicMin(slot, (z << 12) | (unsigned long long)u);
  }
}

// grid (ceil(S / 256)): the pick of slot[t] is recorded and m lowered by its row
__global__ void __launch_bounds__(256)
k_red_update(const long long* __restrict__ dist, int S, const unsigned long long* __restrict__ slot, unsigned long long* __restrict__ m,
             unsigned char* __restrict__ selected, int* __restrict__ chosen, long long* __restrict__ cost) {
  const unsigned long long key = *slot;
  const int u = (int)(key & 0xFFFull), j = blockIdx.x * 256 + threadIdx.x;
  if (key == RD_RED_EMPTY || u >= S) return;                               // (no candidate was left: k <= S rules it out)
  if (j < S) {
    const unsigned long long d = (unsigned long long)dist[(long)u * S + j];
    if (d < m[j]) m[j] = d;
  }
  if (j == 0) *chosen = u, *cost = (long long)(key >> 12), selected[u] = 1;
}

// grid (ceil(S / 256)): counts is zeroed before the launch
__global__ void __launch_bounds__(256)
k_red_assign(const long long* __restrict__ dist, int S, int k, const int* __restrict__ chosen, int* __restrict__ assign, int* __restrict__ counts) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= S) return;
  unsigned long long best = RD_RED_EMPTY;
  int bt = 0;
  for (int t = 0; t < k; ++t) {
    const int u = chosen[t];
    if (u < 0 || u >= S) continue;
    const unsigned long long key = ((unsigned long long)dist[(long)u * S + j] << 12) | (unsigned long long)u;
    if (key < best) best = key, bt = t;
  }
  assign[j] = (int)(best & 0xFFFull);
  atomicAdd(&counts[bt], 1);
}
