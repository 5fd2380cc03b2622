// Random-cascade baseline: the microcanonical multiplicative cascade of Olsson (1998) with the three-way first
// split of a 24-hour day (Mueller & Haberlandt 2015).  Calibration counts, over observed hourly data, how a wet box of rain splits
// into its parts; generation applies those splits recursively to a daily sum: 24 h -> 3 x 8 h -> 4 h -> 2 h -> 1 h.
// Everything is an integer.  q = (int) rintf(x * 1024) in units of 2^-10 mm; a pixel-hour is bad when x is NaN, +-inf, negative or
// >= 2048.  A pixel-day with a bad hour is left out whole (n_bad), one with sum 0 adds nothing else (n_dry).
//
// The tree of a pixel-day has 22 split nodes: node 0 the day (thirds of 8 h), nodes 1 .. 3 the 8 h boxes (level 0), 4 .. 9 the 4 h
// boxes (level 1), 10 .. 21 the 2 h boxes (level 2), each of the last three levels split into halves.  A node of volume 0 is not a
// sample.  Volume class of a box of `hours` hours: the number of edges e (integers per hour, at most 7) with V >= e * hours; NV =
// edges + 1.  Position class of a box of a binary level, from the wetness of the previous and the next box of its level within the
// day (beyond the day's ends: dry): 0 isolated, 1 starting, 2 enclosed, 3 ending.  Type of a binary split: 0 = 0/1 (first half dry),
// 1 = 1/0, 2 = x/(1-x) with the weight bin b = (V1 * 32) / V.
//
// Flat state, 64-bit counters (the model table has the same layout, 32-bit thresholds, without the last three words):
//     type    [3][4][NV][3]     at 0          weight  [3][4][NV][32]    at 36 NV
//     pattern [NV][8]           at 420 NV     w2      [NV][8][32]       at 428 NV     (bit t of a pattern: third t is wet)
//     w3a     [NV][32]          at 684 NV     w3b     [NV][32]          at 716 NV
//     n_days, n_bad, n_dry      at 748 NV     (pixel-days)
// Kernels.
//  * k_cascade_accumulate<VEC>: the only read of the hourly array.  A lane takes VEC adjacent pixels of a day and walks the 24 hours
//    (one 16-byte load an hour for VEC = 4, a scalar load for VEC = 1; adjacent lanes, adjacent pixels), leaves a dry or bad
//    pixel-day at once, and otherwise forms the tree sums in registers, classifies the 22 nodes and increments the workgroup's own
//    counters in LDS (32-bit integer atomics; a workgroup makes fewer than 2^32 increments).  The non-zero counters go to the state
//    with 64-bit integer atomics at the end.  Integer sums: the state does not depend on the grid or on how days are grouped.
//  * k_cascade_generate<VEC>: the model table is copied to LDS once per workgroup; a lane takes VEC adjacent pixels of one (query,
//    member), walks the tree level by level in registers and stores the 24 planes (16-byte stores for VEC = 4).
// No floating-point atomic, no spin-wait, no grid sync.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_rng.h"
#include "rdgan_hourly.hip.h"

#define RD_CS_NB 32                      // weight bins
#define RD_CS_NP 4                       // position classes
#define RD_CS_NL 3                       // binary levels
#define RD_CS_NT 3                       // types of a binary split
#define RD_CS_MAXE 7                     // edges of the volume classes
#define RD_CS_PER_CLASS 748              // counters per volume class
#define RD_CS_TAIL 3                     // n_days, n_bad, n_dry
#define RD_CS_MAXEDGE (1 << 21)          // an edge in units per hour: 2048 mm/h
#define RD_CS_MAXQ (1L << 18)            // queries of a call
#define RD_CS_MAXS 65535                 // members of a call
#define RD_CS_MAXCOND 16384              // a condition at or above it is masked: V = rd_depth_q(cond) < 2^24
#define RD_CS_THREADS 256
#define RD_CS_ACC_MAXBLOCKS 2048         // workgroups of an accumulate call: 2^40 / 24 pixel-days over them is below 2^25 each
#define RD_CS_GEN_MAXBLOCKS 8192
#define RD_CS_NODE_DAY2 22               // the draws of a three-wet day's second split
// RD_HOURLY_MAXPLANE pixels of a plane: a draw's counter (block * 32 + node) * 4 + draw stays below 2^31; RD_HOURLY_MAXELEMS bounds
// one call's hourly array, and one call's output
static_assert(RD_HOURLY_MAXPLANE * 32 * 4 <= (1L << 31) && RD_CS_MAXCOND * RD_DEPTH_UNIT <= (1 << 24), "the draw counter and V");

struct rd_cs_edges {
  int n;
  int v[RD_CS_MAXE];
};

__host__ __device__ inline long rd_cs_state_size(int n_edges) { return (long)RD_CS_PER_CLASS * (n_edges + 1) + RD_CS_TAIL; }
__host__ __device__ inline int rd_cs_off_weight(int NV) { return 36 * NV; }
__host__ __device__ inline int rd_cs_off_pattern(int NV) { return 420 * NV; }
__host__ __device__ inline int rd_cs_off_w2(int NV) { return 428 * NV; }
__host__ __device__ inline int rd_cs_off_w3a(int NV) { return 684 * NV; }
__host__ __device__ inline int rd_cs_off_w3b(int NV) { return 716 * NV; }
__host__ __device__ inline int rd_cs_off_tail(int NV) { return RD_CS_PER_CLASS * NV; }

__device__ __forceinline__ int rd_cs_vclass(unsigned V, const rd_cs_edges& e, unsigned hours) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < RD_CS_MAXE; ++i) c += (i < e.n && V >= (unsigned)e.v[i] * hours) ? 1 : 0;
  return c;
}

__device__ __forceinline__ int rd_cs_pos(bool prev, bool next) { return prev ? (next ? 2 : 3) : (next ? 1 : 0); }

// (a * 32) / V for a <= V, 0 < V <= 2^26: the float estimate is off by one at most, the products decide (32 V <= 2^31)
__device__ __forceinline__ unsigned rd_cs_bin(unsigned a, unsigned V) {
  const unsigned n = a * RD_CS_NB;
  unsigned b = (unsigned)((float)n * __builtin_amdgcn_rcpf((float)V));
  b = min(b, (unsigned)RD_CS_NB);
  while (b * V > n) --b;
  while ((b + 1u) * V <= n) ++b;
  return b;
}

// the boxes of a binary level and their halves: a type counter per wet box, a weight counter per x/(1-x) split
template <int NBOX>
__device__ __forceinline__ void rd_cs_count_level(const unsigned (&box)[NBOX], const unsigned (&half)[2 * NBOX], int level, unsigned hours,
                                                  const rd_cs_edges& e, int NV, unsigned* cnt) {
#pragma unroll
  for (int j = 0; j < NBOX; ++j) {
    const unsigned V = box[j];
    if (V == 0u) continue;
    const bool prev = j > 0 && box[j > 0 ? j - 1 : 0] > 0u, next = j + 1 < NBOX && box[j + 1 < NBOX ? j + 1 : j] > 0u;
    const int row = (level * RD_CS_NP + rd_cs_pos(prev, next)) * NV + rd_cs_vclass(V, e, hours);
    const unsigned V1 = half[2 * j];
    const int t = V1 == 0u ? 0 : (V1 == V ? 1 : 2);
    atomicAdd(&cnt[row * RD_CS_NT + t], 1u);
    if (t == 2) atomicAdd(&cnt[rd_cs_off_weight(NV) + row * RD_CS_NB + (int)rd_cs_bin(V1, V)], 1u);
  }
}

// one wet pixel-day: q the 24 hours, D > 0 their sum
__device__ __forceinline__ void rd_cs_count_day(const unsigned (&q)[RD_HOURS], unsigned D, const rd_cs_edges& e, int NV, unsigned* cnt) {
  unsigned v2[12], v4[6], v8[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) v2[i] = q[2 * i] + q[2 * i + 1];
#pragma unroll
  for (int i = 0; i < 6; ++i) v4[i] = v2[2 * i] + v2[2 * i + 1];
#pragma unroll
  for (int i = 0; i < 3; ++i) v8[i] = v4[2 * i] + v4[2 * i + 1];
  const int vc = rd_cs_vclass(D, e, RD_HOURS);
  const int pat = (v8[0] > 0u ? 1 : 0) | (v8[1] > 0u ? 2 : 0) | (v8[2] > 0u ? 4 : 0);
  atomicAdd(&cnt[rd_cs_off_pattern(NV) + vc * 8 + pat], 1u);
  if (pat == 7) {
    atomicAdd(&cnt[rd_cs_off_w3a(NV) + vc * RD_CS_NB + (int)rd_cs_bin(v8[0], D)], 1u);
    atomicAdd(&cnt[rd_cs_off_w3b(NV) + vc * RD_CS_NB + (int)rd_cs_bin(v8[1], D - v8[0])], 1u);
  } else if (pat == 3 || pat == 5 || pat == 6) {
    atomicAdd(&cnt[rd_cs_off_w2(NV) + (vc * 8 + pat) * RD_CS_NB + (int)rd_cs_bin((pat & 1) ? v8[0] : v8[1], D)], 1u);
  }
  rd_cs_count_level<3>(v8, v4, 0, 8u, e, NV, cnt);
  rd_cs_count_level<6>(v4, v2, 1, 4u, e, NV, cnt);
  rd_cs_count_level<12>(v2, q, 2, 2u, e, NV, cnt);
}

// grid (<= RD_CS_ACC_MAXBLOCKS), grid-stride over the items = day * (plane / VEC) + pixel group; dynamic LDS rd_cs_state_size * 4
// bytes.  VEC = 4 needs x 16-byte aligned and plane and day_stride multiples of 4.
template <int VEC>
__global__ void __launch_bounds__(RD_CS_THREADS)
k_cascade_accumulate(const float* __restrict__ x, long n, long day_stride, long plane, rd_cs_edges e, unsigned long long* __restrict__ state) {
  extern __shared__ __attribute__((aligned(16))) unsigned rd_cs_cnt[];
  const int tid = threadIdx.x, NV = e.n + 1, total = (int)rd_cs_state_size(e.n);
  for (int i = tid; i < total; i += RD_CS_THREADS) rd_cs_cnt[i] = 0u;
  __syncthreads();
  const long groups = plane / VEC, items = n * groups;
  unsigned n_bad = 0u, n_dry = 0u;
  for (long item = (long)blockIdx.x * RD_CS_THREADS + tid; item < items; item += (long)gridDim.x * RD_CS_THREADS) {
    const long j = item / groups;
    const float* xd = x + j * day_stride + (item - j * groups) * VEC;
    unsigned q[VEC][RD_HOURS], D[VEC];
    bool bad[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) D[k] = 0u, bad[k] = false;
#pragma unroll
    for (int h = 0; h < RD_HOURS; ++h) {
      float v[VEC];
      rd_load<VEC>(xd + (long)h * plane, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool b = rd_depth_bad(v[k]);
        q[k][h] = b ? 0u : (unsigned)rd_depth_q(v[k]);
        D[k] += q[k][h];
        bad[k] |= b;
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (bad[k]) ++n_bad;
      else if (D[k] == 0u) ++n_dry;
      else rd_cs_count_day(q[k], D[k], e, NV, rd_cs_cnt);
    }
  }
  for (int s = 32; s > 0; s >>= 1) n_bad += __shfl_xor(n_bad, s), n_dry += __shfl_xor(n_dry, s);
  if ((tid & 63) == 0) {
    if (n_bad) atomicAdd(&rd_cs_cnt[rd_cs_off_tail(NV) + 1], n_bad);
    if (n_dry) atomicAdd(&rd_cs_cnt[rd_cs_off_tail(NV) + 2], n_dry);
  }
  __syncthreads();
  for (int i = tid; i < total; i += RD_CS_THREADS) {
    const unsigned c = rd_cs_cnt[i];
    if (c) atomicAdd(&state[i], (unsigned long long)c);
  }
  if (blockIdx.x == 0 && tid == 0) atomicAdd(&state[rd_cs_off_tail(NV)], (unsigned long long)(n * plane));
}

// ---- generation
__device__ __forceinline__ unsigned rd_cs_draw(uint32_t key, unsigned block, int node, int d) {
  return rd_bits(key, (block * 32u + (unsigned)node) * 4u + (unsigned)d) >> 8;
}

// the first j with row[j] > r in a row of 32 non-decreasing thresholds whose last is 2^24 > r; five reads, and inside the row whatever it holds
__device__ __forceinline__ unsigned rd_cs_pick32(const unsigned* row, unsigned r) {
  unsigned lo = 0u;
#pragma unroll
  for (unsigned s = 16u; s > 0u; s >>= 1)
    if (row[lo + s - 1u] <= r) lo += s;
  return lo;
}

// clamp((V * ((b << 24) + u)) >> 29, 1, most): V < 2^24, the product below 2^53
__device__ __forceinline__ unsigned rd_cs_part(unsigned V, unsigned b, unsigned u, unsigned most) {
  const unsigned v1 = (unsigned)(((unsigned long long)V * (((unsigned long long)b << 24) + u)) >> 29);
  return min(max(v1, 1u), most);
}

// the halves of the boxes of a binary level; node0 the level's first node
template <int NBOX>
__device__ __forceinline__ void rd_cs_split_level(const unsigned (&box)[NBOX], unsigned (&half)[2 * NBOX], int level, int node0, unsigned hours,
                                                  uint32_t key, unsigned block, const rd_cs_edges& e, int NV, const unsigned* tab) {
#pragma unroll
  for (int j = 0; j < NBOX; ++j) {
    const unsigned V = box[j];
    unsigned V1 = 0u;
    if (V > 0u) {
      const bool prev = j > 0 && box[j > 0 ? j - 1 : 0] > 0u, next = j + 1 < NBOX && box[j + 1 < NBOX ? j + 1 : j] > 0u;
      const int row = (level * RD_CS_NP + rd_cs_pos(prev, next)) * NV + rd_cs_vclass(V, e, hours);
      const unsigned c0 = tab[row * RD_CS_NT], c1 = tab[row * RD_CS_NT + 1];
      const unsigned r = rd_cs_draw(key, block, node0 + j, 0);
      int t;
      if (V >= 2u) t = r < c0 ? 0 : (r < c1 ? 1 : 2);
      else if (c1 == 0u) t = (int)(r >> 23);                             // V = 1 cannot split x/(1-x): the two other types in their own
      else t = (unsigned)(((unsigned long long)r * c1) >> 24) < c0 ? 0 : 1;       // proportion, evenly where they have no mass
      if (t == 2) {
        const unsigned b = rd_cs_pick32(tab + rd_cs_off_weight(NV) + row * RD_CS_NB, rd_cs_draw(key, block, node0 + j, 1));
        V1 = rd_cs_part(V, b, rd_cs_draw(key, block, node0 + j, 2), V - 1u);
      } else {
        V1 = t == 1 ? V : 0u;
      }
    }
    half[2 * j] = V1, half[2 * j + 1] = V - V1;
  }
}

// one pixel of volume V > 0 -> its 24 hours
__device__ __forceinline__ void rd_cs_walk(unsigned V, uint32_t key, unsigned block, const rd_cs_edges& e, int NV, const unsigned* tab,
                                           unsigned (&q)[RD_HOURS]) {
  unsigned v8[3], v4[6], v2[12];
  const int vc = rd_cs_vclass(V, e, RD_HOURS);
  const unsigned* prow = tab + rd_cs_off_pattern(NV) + vc * 8;
  const unsigned r = rd_cs_draw(key, block, 0, 0);
  int pat = 7;
#pragma unroll
  for (int j = 6; j >= 1; --j) pat = prow[j] > r ? j : pat;              // the first j with c[j] > r (c[0] = 0: pattern 0 never)
  if (V == 1u) pat &= -pat;                                              // more wet thirds than units: the highest are dropped
  else if (V == 2u && pat == 7) pat = 3;
  if (pat == 7) {
    const unsigned b1 = rd_cs_pick32(tab + rd_cs_off_w3a(NV) + vc * RD_CS_NB, rd_cs_draw(key, block, 0, 1));
    v8[0] = rd_cs_part(V, b1, rd_cs_draw(key, block, 0, 2), V - 2u);
    const unsigned R = V - v8[0];
    const unsigned b2 = rd_cs_pick32(tab + rd_cs_off_w3b(NV) + vc * RD_CS_NB, rd_cs_draw(key, block, RD_CS_NODE_DAY2, 1));
    v8[1] = rd_cs_part(R, b2, rd_cs_draw(key, block, RD_CS_NODE_DAY2, 2), R - 1u);
    v8[2] = R - v8[1];
  } else if (pat == 3 || pat == 5 || pat == 6) {
    const unsigned b = rd_cs_pick32(tab + rd_cs_off_w2(NV) + (vc * 8 + pat) * RD_CS_NB, rd_cs_draw(key, block, 0, 1));
    const unsigned first = rd_cs_part(V, b, rd_cs_draw(key, block, 0, 2), V - 1u), second = V - first;
    v8[0] = (pat & 1) ? first : 0u;
    v8[1] = pat == 3 ? second : (pat == 6 ? first : 0u);
    v8[2] = (pat & 4) ? second : 0u;
  } else {
    v8[0] = pat == 1 ? V : 0u, v8[1] = pat == 2 ? V : 0u, v8[2] = pat == 4 ? V : 0u;
  }
  rd_cs_split_level<3>(v8, v4, 0, 1, 8u, key, block, e, NV, tab);
  rd_cs_split_level<6>(v4, v2, 1, 4, 4u, key, block, e, NV, tab);
  rd_cs_split_level<12>(v2, q, 2, 10, 2u, key, block, e, NV, tab);
}

// grid (<= RD_CS_GEN_MAXBLOCKS), grid-stride over the items = ((query * S + member) * (plane / VEC)) + pixel group; dynamic LDS
// RD_CS_PER_CLASS * NV * 4 bytes.  out, units [Q][S][24][plane]; units may be null.  VEC = 4 needs nx a multiple of 4 and out and
// units 16-byte aligned.  nbx = ceil(nx / patch).
template <int VEC>
__global__ void __launch_bounds__(RD_CS_THREADS)
k_cascade_generate(const unsigned* __restrict__ model, rd_cs_edges e, const float* __restrict__ cond, long Q, long first_query, int nx,
                   long plane, long S, long first_member, unsigned long long seed, int patch, int nbx, float* __restrict__ out,
                   int* __restrict__ units) {
  extern __shared__ __attribute__((aligned(16))) unsigned rd_cs_tab[];
  const int tid = threadIdx.x, NV = e.n + 1;
  for (int i = tid; i < RD_CS_PER_CLASS * NV; i += RD_CS_THREADS) rd_cs_tab[i] = model[i];
  __syncthreads();
  const long groups = plane / VEC, items = Q * S * groups;
  const uint32_t base = rd_make_key(seed, RD_STREAM_CASCADE);
  for (long item = (long)blockIdx.x * RD_CS_THREADS + tid; item < items; item += (long)gridDim.x * RD_CS_THREADS) {
    const long qm = item / groups, i = qm / S, m = qm - i * S;
    const int p0 = (int)(item - qm * groups) * VEC;
    const uint32_t key = rd_member_key(rd_member_key(base, (uint64_t)(first_member + m)), (uint64_t)(first_query + i));
    unsigned u[RD_HOURS][VEC];                                        // units; ~0 for a masked pixel
#pragma unroll
    for (int h = 0; h < RD_HOURS; ++h) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) u[h][k] = 0u;
    }
#pragma unroll 1
    for (int k = 0; k < VEC; ++k) {
      const int p = p0 + k, y = p / nx, xx = p - y * nx;
      const float c = cond[i * plane + p];
      unsigned q[RD_HOURS];
      if (!(c >= 0.0f && c < (float)RD_CS_MAXCOND)) {
#pragma unroll
        for (int h = 0; h < RD_HOURS; ++h) q[h] = ~0u;
      } else {
        const unsigned V = (unsigned)rd_depth_q(c);
#pragma unroll
        for (int h = 0; h < RD_HOURS; ++h) q[h] = 0u;
        if (V > 0u) rd_cs_walk(V, key, (unsigned)((y / patch) * nbx + xx / patch), e, NV, rd_cs_tab, q);
      }
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) {
#pragma unroll
        for (int kk = 0; kk < VEC; ++kk) u[h][kk] = kk == k ? q[h] : u[h][kk];
      }
    }
    const float nan = __builtin_nanf("");
    const long o0 = qm * RD_HOURS * plane + p0;
#pragma unroll
    for (int h = 0; h < RD_HOURS; ++h) {
      float f[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) f[k] = u[h][k] == ~0u ? nan : (float)u[h][k] * (1.0f / (float)RD_DEPTH_UNIT);
      if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(out + o0 + (long)h * plane) = make_float4(f[0], f[1], f[2], f[3]);
        if (units) *reinterpret_cast<int4*>(units + o0 + (long)h * plane) = make_int4((int)u[h][0], (int)u[h][1], (int)u[h][2], (int)u[h][3]);
      } else {
        out[o0 + (long)h * plane] = f[0];
        if (units) units[o0 + (long)h * plane] = (int)u[h][0];
      }
    }
  }
}
