// Analog baseline, the method of fragments: for a daily condition the k library days whose daily field
// most resembles it, one of them picked per member, its hourly fractions scaled to the condition's daily amounts.
// Everything of the search is an integer.  q = (int) rintf(x * 1024) in units of 2^-10 mm; a pixel-hour of the library is bad
// when x is NaN, +-inf, negative or >= 2048; D[p] = sum of q over the 24 hours < 2^26; the feature is e[p] = floor(sqrt(D[p])) <
// 2^13, a uint16.  A library day is void when it holds a bad pixel-hour or its total is 0; a void day is never a neighbour.  A
// query pixel is masked when x is NaN, +-inf, negative or >= 2048 * 24, and adds nothing to any distance of its query.
// dist(i, j) = sum over the unmasked pixels of (e_i - e_j)^2 < 2^38; key = dist 2^24 + j < 2^62, so equal distances go to the
// smaller library index and every key of a query is distinct: the k smallest keys are one set, whatever order they are met in.
//
// Layouts.  P = ny nx pixels, padded to Ppad = 8 ceil(P / 8); a CHUNK is 8 pixels, 16 bytes of features; C = Ppad / 8.
//  * library features: blocks of 64 days; the chunk c of the day j lies at uint4 index ((j / 64) C + c) 64 + j % 64 -- the 64
//    lanes of a wave, one day each, read one chunk of their block as 1 KB of consecutive bytes.  64 ceil(N / 64) Ppad 2 bytes.
//  * query features and masks: [Q][Ppad] uint16 each; a mask word is 0xFFFF for a pixel that counts, 0 for a masked or padding
//    pixel, where the feature is 0 too: (e_i - (e_j & mask))^2 is then 0.
//  * the workspace of a search: lists [Q][L][k] of 64-bit keys, L = slices x 8 waves, ~0 for an empty slot.
// Kernels.
//  * k_analog_features<VEC>: the only read of the hourly library.  One thread per chunk of a day walks the 24 hours (two 16-byte
//    loads an hour where the plane allows, eight guarded scalar loads where not), writes the chunk's features and adds the
//    chunk's total, and 2^40 if it met a bad pixel-hour, to the day's word; k_analog_days turns the words into totals and void
//    flags and counts the void days.  k_analog_query does the same for the conditions, with the mask.
//  * k_analog_search<QT>: grid (slices, query tiles).  A workgroup of 8 waves holds QT queries' features and masks in LDS and
//    streams its slice of the library past them, a block of 64 days per wave and step, one day per lane: the library's bytes are
//    read once per query tile.  Two pixels per instruction: v_and, v_pk_sub_i16, v_dot2c_i32_i16 (the differences fit 14 bits);
//    the 32-bit sum is added to a 64-bit one every 64 pixels, 64 * 8191^2 < 2^32.  Each wave keeps, per query, the 64 smallest
//    keys seen, sorted across its lanes, and inserts a block's candidates below the k-th one by one; it writes the first k.
//  * k_analog_merge: one wave per query folds the L lists the same way and writes neighbours, distances, found.
//  * k_analog_apply: one workgroup per (query, member): the pick from the counter RNG, the donor's pixel sums (fp32, hours in
//    order) into LDS and its areal profile (fp64 sums), then the scaled fractions.
// Kernel boundaries are the only ordering between the phases: no spin-wait, no grid sync, no floating-point atomic.  All global
// offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_rng.h"
#include "rdgan_hourly.hip.h"

#define RD_AN_MAXP 4096                  // pixels of a plane
#define RD_AN_MAXN ((1L << 24) - 1)      // library days: the index takes the low 24 bits of a key
#define RD_AN_MAXQ (1L << 18)            // queries of a call
#define RD_AN_MAXK 32                    // neighbours
#define RD_AN_MAXS 65535                 // members of a call: the grid's y
#define RD_AN_BLOCK 64                   // days of a block: one per lane
#define RD_AN_THREADS 512                // of the search kernel
#define RD_AN_WAVES 8
#define RD_AN_QT_SMALL 16                // queries of a tile while Ppad <= RD_AN_QT_SPLIT: at most 16 * 2048 * 4 = 128 KB of LDS
#define RD_AN_QT_LARGE 8                 // above: at most 8 * 4096 * 4 = 128 KB
#define RD_AN_QT_SPLIT 2048
#define RD_AN_WIDEN 8                    // chunks between two additions to the 64-bit sums: 64 pixels
#define RD_AN_BADBIT 40                  // of a day's word: chunks with a bad pixel-hour are counted from this bit up
#define RD_AN_EMPTY (~0ull)
#define RD_AN_APPLY_THREADS 256
#define RD_AN_UNIFORM 0
#define RD_AN_RANK 1

__host__ __device__ inline long rd_an_ppad(long plane) { return (plane + 7) / 8 * 8; }
__host__ __device__ inline long rd_an_blocks(long n) { return (n + RD_AN_BLOCK - 1) / RD_AN_BLOCK; }
__host__ __device__ inline int rd_an_query_tile(long plane) { return rd_an_ppad(plane) <= RD_AN_QT_SPLIT ? RD_AN_QT_SMALL : RD_AN_QT_LARGE; }
__host__ __device__ inline size_t rd_an_lds_bytes(long plane) { return (size_t)rd_an_query_tile(plane) * rd_an_ppad(plane) * 4; }
__host__ __device__ inline long rd_an_list_bytes(long n_queries, int k) { return n_queries * RD_AN_WAVES * k * 8; }   // per slice

// floor(sqrt(D)) for D < 2^27: the float estimate is off by one at most, the squares decide
__device__ __forceinline__ unsigned rd_an_isqrt(unsigned D) {
  unsigned r = (unsigned)sqrtf((float)D);
  while (r * r > D) --r;
  while ((r + 1u) * (r + 1u) <= D) ++r;
  return r;
}

// grid (ceil(n C / 256)); item = day * C + chunk.  VEC needs x 16-byte aligned and plane and day_stride multiples of 4.
template <bool VEC>
__global__ void __launch_bounds__(256)
k_analog_features(const float* __restrict__ x, long n, long day_stride, int plane, int C, uint4* __restrict__ feat,
                  unsigned long long* __restrict__ words) {
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  const bool active = item < n * C;
  const long j = active ? item / C : 0;
  const int c = active ? (int)(item - j * C) : 0, p0 = c * 8;
  unsigned long long word = 0ull;
  if (active) {
    const float* xd = x + j * day_stride + p0;
    unsigned sum[8];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) sum[i] = 0u;
#pragma unroll 4
    for (int h = 0; h < RD_HOURS; ++h) {
      float v[8];
      if constexpr (VEC) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (p0 < plane) a = *reinterpret_cast<const float4*>(xd + (long)h * plane);
        if (p0 + 4 < plane) b = *reinterpret_cast<const float4*>(xd + (long)h * plane + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p0 + i < plane ? xd[(long)h * plane + i] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool b = rd_depth_bad(v[i]);
        sum[i] += b ? 0u : (unsigned)rd_depth_q(v[i]);
        bad |= b;
      }
    }
    unsigned e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = rd_an_isqrt(sum[i]), word += sum[i];
    if (bad) word += 1ull << RD_AN_BADBIT;
    feat[((j / RD_AN_BLOCK) * C + c) * RD_AN_BLOCK + j % RD_AN_BLOCK] =
        make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16);
  }
  // the chunks of a day that share a wave add up first: C a power of two below 64 puts 64 / C whole days into a wave
  const int span = (C & (C - 1)) == 0 ? min(C, 64) : 1;
  for (int s = 1; s < span; s <<= 1) word += __shfl_xor(word, s);
  if (active && (threadIdx.x & (span - 1)) == 0 && word) atomicAdd(&words[j], word);
}

// grid (ceil(n / 256)): words -> totals (the sum of q over the pixel-hours that are not bad) and void flags; counts the void days
__global__ void __launch_bounds__(256)
k_analog_days(long n, unsigned long long* __restrict__ words, unsigned char* __restrict__ voids, unsigned long long* __restrict__ n_void) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  bool v = false;
  if (j < n) {
    const unsigned long long w = words[j], total = w & ((1ull << RD_AN_BADBIT) - 1);
    v = (w >> RD_AN_BADBIT) != 0ull || total == 0ull;
    words[j] = total;
    voids[j] = v ? 1 : 0;
  }
  const unsigned long long m = __ballot(v);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_void, (unsigned long long)__popcll(m));
}

// grid (ceil(n Ppad / 256)): the conditions [n][plane] -> features and masks [n][Ppad]
__global__ void __launch_bounds__(256)
k_analog_query(const float* __restrict__ x, long n, int plane, int ppad, unsigned short* __restrict__ feat, unsigned short* __restrict__ mask) {
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= n * ppad) return;
  const long i = item / ppad;
  const int p = (int)(item - i * ppad);
  unsigned e = 0u, m = 0u;
  if (p < plane) {
    const float v = x[i * plane + p];
    if (v >= 0.0f && v < (float)RD_DEPTH_MAX * RD_HOURS) e = rd_an_isqrt((unsigned)rd_depth_q(v)), m = 0xFFFFu;
  }
  feat[item] = (unsigned short)e;
  mask[item] = (unsigned short)m;
}

// two pixels: acc + (e.lo - f.lo)^2 + (e.hi - f.hi)^2, modulo 2^32
__device__ __forceinline__ unsigned rd_an_sq2(unsigned e, unsigned f, unsigned acc) {
  typedef short rd_an_s2 __attribute__((ext_vector_type(2)));
  const rd_an_s2 d = __builtin_bit_cast(rd_an_s2, e) - __builtin_bit_cast(rd_an_s2, f);
  return (unsigned)__builtin_amdgcn_sdot2(d, d, (int)acc, false);
}

// `list` holds, across the 64 lanes of a wave, the smallest keys seen in ascending order (~0: none).  Every lane offers `key`
// if `ok`; the keys below the k-th of the list go in one at a time, the threshold falling as they do.  Wave-uniform control flow.
__device__ __forceinline__ void rd_an_insert(unsigned long long& list, unsigned long long key, bool ok, int k, int lane) {
  unsigned long long thr = __shfl(list, k - 1);
  unsigned long long cand = __ballot(ok && key < thr);
  while (cand) {
    const int src = __ffsll((long long)cand) - 1;
    cand &= cand - 1ull;
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(key >> 32), src), lo = (unsigned)__builtin_amdgcn_readlane((int)key, src);
    const unsigned long long x = ((unsigned long long)hi << 32) | lo;     // (the builtin returns a signed int: no sign extension)
    const unsigned long long up = __shfl_up(list, 1);
    const bool here = lane == 0 || up < x;
    list = list < x ? list : (here ? x : up);
    thr = __shfl(list, k - 1);
    cand &= __ballot(ok && key < thr);
  }
}

// grid (slices, ceil(Q / QT)); dynamic LDS QT * C * 32 bytes: [c][q] {features, mask} as uint4 pairs.
// lists [Q][L][k], L = gridDim.x * 8: the wave w of the slice s writes the list s * 8 + w of each of its queries.
template <int QT>
__global__ void __launch_bounds__(RD_AN_THREADS)
k_analog_search(const uint4* __restrict__ feat, const unsigned char* __restrict__ voids, const int* __restrict__ lib_groups,
                const uint4* __restrict__ qfeat, const uint4* __restrict__ qmask, const int* __restrict__ query_groups, int N, int Q, int C,
                int k, int nblocks, int blocks_per_slice, unsigned long long* __restrict__ lists) {
  extern __shared__ __attribute__((aligned(16))) uint4 rd_an_qs[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * QT;
  for (int i = tid; i < QT * C; i += RD_AN_THREADS) {
    const int c = i / QT, q = i - c * QT;
    uint4 e = make_uint4(0u, 0u, 0u, 0u), m = e;
    if (q0 + q < Q) e = qfeat[(long)(q0 + q) * C + c], m = qmask[(long)(q0 + q) * C + c];
    rd_an_qs[2 * i] = e, rd_an_qs[2 * i + 1] = m;
  }
  __syncthreads();
  unsigned long long list[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) list[q] = RD_AN_EMPTY;
  const int b0 = blockIdx.x * blocks_per_slice, b1 = min(b0 + blocks_per_slice, nblocks);
  const bool grouped = lib_groups && query_groups;
  for (int b = b0 + wave; b < b1; b += RD_AN_WAVES) {
    const uint4* fb = feat + (long)b * C * RD_AN_BLOCK + lane;
    unsigned acc[QT];
    unsigned long long tot[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = 0u, tot[q] = 0ull;
    uint4 f = fb[0];
    for (int c0 = 0; c0 < C; c0 += RD_AN_WIDEN) {
      const int c1 = min(c0 + RD_AN_WIDEN, C);
      for (int c = c0; c < c1; ++c) {
        const uint4 next = fb[(long)min(c + 1, C - 1) * RD_AN_BLOCK];
        const uint4* qc = rd_an_qs + 2 * c * QT;
#pragma unroll
        for (int q = 0; q < QT; ++q) {
          const uint4 e = qc[2 * q], m = qc[2 * q + 1];
          unsigned a = acc[q];
          a = rd_an_sq2(e.x, f.x & m.x, a);
          a = rd_an_sq2(e.y, f.y & m.y, a);
          a = rd_an_sq2(e.z, f.z & m.z, a);
          a = rd_an_sq2(e.w, f.w & m.w, a);
          acc[q] = a;
        }
        f = next;
      }
#pragma unroll
      for (int q = 0; q < QT; ++q) tot[q] += acc[q], acc[q] = 0u;
    }
    const int j = b * RD_AN_BLOCK + lane;
    const bool live = j < N && !voids[j];
    const int g = live && grouped ? lib_groups[j] : -1;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      if (q0 + q >= Q) break;                                              // (uniform)
      const bool ok = live && !(g >= 0 && query_groups[q0 + q] == g);
      rd_an_insert(list[q], (tot[q] << 24) | (unsigned long long)(unsigned)j, ok, k, lane);
    }
  }
  const long L = (long)gridDim.x * RD_AN_WAVES;
  if (lane < k) {
#pragma unroll
    for (int q = 0; q < QT; ++q)
      if (q0 + q < Q) lists[(((long)(q0 + q)) * L + (long)blockIdx.x * RD_AN_WAVES + wave) * k + lane] = list[q];
  }
}

// grid (Q), one wave: lists [Q][L][k] -> neighbours, distances [Q][k] (-1: none), found [Q]
__global__ void __launch_bounds__(64)
k_analog_merge(const unsigned long long* __restrict__ lists, long L, int k, int* __restrict__ neighbours, long long* __restrict__ distances,
               int* __restrict__ found) {
  const int lane = threadIdx.x;
  const long q = blockIdx.x, count = L * k;
  const unsigned long long* mine = lists + q * count;
  unsigned long long list = RD_AN_EMPTY;
  for (long i = 0; i < count; i += 64) {
    const unsigned long long key = i + lane < count ? mine[i + lane] : RD_AN_EMPTY;
    rd_an_insert(list, key, key != RD_AN_EMPTY, k, lane);
  }
  const bool have = lane < k && list != RD_AN_EMPTY;
  if (lane < k) {
    neighbours[q * k + lane] = have ? (int)(list & 0xFFFFFFull) : -1;
    distances[q * k + lane] = have ? (long long)(list >> 24) : -1ll;
  }
  const unsigned long long m = __ballot(have);
  if (lane == 0) found[q] = __popcll(m);
}

// the rank of the pick among f neighbours from 32 random bits
__host__ __device__ inline int rd_an_pick_rank(unsigned bits, int f, int weights) {
  if (weights == RD_AN_UNIFORM) return (int)(((unsigned long long)bits * (unsigned long long)f) >> 32);
  unsigned long long total = 0ull;
  for (int s = 0; s < f; ++s) total += (1u << 20) / (unsigned)(s + 1);
  const unsigned long long target = ((unsigned long long)bits * total) >> 32;
  unsigned long long c = 0ull;
  for (int r = 0; r < f; ++r) {
    c += (1u << 20) / (unsigned)(r + 1);
    if (c > target) return r;
  }
  return f - 1;                                                            // (not reached: target < total)
}

// grid (Q, S); dynamic LDS plane * 4 bytes.  out [Q][S][24][plane], picks [Q][S].
__global__ void __launch_bounds__(RD_AN_APPLY_THREADS)
k_analog_apply(const float* __restrict__ lib, long n, long day_stride, int plane, const float* __restrict__ cond, long first_query,
               const int* __restrict__ neighbours, const int* __restrict__ found, int k, long first_member, unsigned long long seed,
               int weights, float* __restrict__ out, int* __restrict__ picks) {
  extern __shared__ __attribute__((aligned(16))) float rd_an_day[];           // the donor's pixel sums
  __shared__ double part[RD_AN_APPLY_THREADS / 64][RD_HOURS];
  __shared__ float profile[RD_HOURS];
  const int tid = threadIdx.x;
  const long i = blockIdx.x, m = blockIdx.y, S = gridDim.y;
  const int f = min(max(found[i], 0), k);
  long j = -1;
  if (f > 0) {
    const uint32_t key = rd_member_key(rd_make_key(seed, RD_STREAM_ANALOG), (uint64_t)(first_member + m));
    j = neighbours[i * k + rd_an_pick_rank(rd_bits(key, (uint32_t)(first_query + i)), f, weights)];
    if (j < 0 || j >= n) j = -1;                                           // (a list that is not the search's: nothing is read)
  }
  if (tid == 0) picks[i * S + m] = (int)j;
  float* o = out + (i * S + m) * RD_HOURS * plane;
  const float* c = cond + i * plane;
  const float nan = __builtin_nanf("");
  if (j < 0) {                                                             // (uniform)
    for (long e = tid; e < (long)RD_HOURS * plane; e += RD_AN_APPLY_THREADS) o[e] = nan;
    return;
  }
  const float* d = lib + j * day_stride;
  double hsum[RD_HOURS];
#pragma unroll
  for (int h = 0; h < RD_HOURS; ++h) hsum[h] = 0.0;
  for (int p = tid; p < plane; p += RD_AN_APPLY_THREADS) {
    float s = 0.0f;
#pragma unroll
    for (int h = 0; h < RD_HOURS; ++h) {
      const float v = d[(long)h * plane + p];
      s += v;
      hsum[h] += (double)v;
    }
    rd_an_day[p] = s;
  }
#pragma unroll
  for (int h = 0; h < RD_HOURS; ++h) {
    double v = hsum[h];
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    if ((tid & 63) == 0) part[tid >> 6][h] = v;
  }
  __syncthreads();
  if (tid < 64) {
    double v = 0.0;
    if (tid < RD_HOURS)
      for (int w = 0; w < RD_AN_APPLY_THREADS / 64; ++w) v += part[w][tid];
    double all = v;
    for (int s = 32; s > 0; s >>= 1) all += __shfl_xor(all, s);
    if (tid < RD_HOURS) profile[tid] = (float)(v / all);                // (all > 0: the donor is not void)
  }
  __syncthreads();
  for (int p = tid; p < plane; p += RD_AN_APPLY_THREADS) {
    const float cv = c[p], dp = rd_an_day[p];
    const bool masked = !(cv >= 0.0f && cv < (float)RD_DEPTH_MAX * RD_HOURS);
#pragma unroll 4
    for (int h = 0; h < RD_HOURS; ++h) {
      const float frac = dp > 0.0f ? d[(long)h * plane + p] / dp : profile[h];
      o[(long)h * plane + p] = masked ? nan : cv * frac;
    }
  }
}
