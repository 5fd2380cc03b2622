// Distance-map verification of hourly fields: the exact Euclidean distance transform of event sets, in
// integers, and the records from which Hausdorff distance, mean error distance, Baddeley's Delta and Zhu's measure are formed on the
// host.  For a threshold u the set of a plane is its pixels with a finite value v > u (fp32 compare); a NaN or +-inf pixel is bad.
//   d2(x, S) = min over a in S of dy^2 + dx^2, an exact integer;  D(x, S) = isqrt(256 d2) = floor(16 sqrt(d2)), 0xFFFF for an empty S.
// Sides are at most RD_DM_MAXSIDE = 2048, so 256 d2 <= 256 * 2 * 2047^2 < 2^31 and D <= 46 318 fits 16 bits.  isqrt(v) is
// floor(sqrt((double)v)): for k < 2^16 the gap k - sqrt(k^2 - 1) exceeds 2^-17, far above an fp64 ulp of a value below 2^16, so the
// correctly rounded root of v < k^2 never reaches k (tests/test_distmap_host.py checks every 256 (dy^2 + dx^2) a plane can produce).
//
//  * k_dm_pack: a wave takes 64 adjacent pixels of a row, the ballot of a compare is the row word.  Per plane T event masks and one
//    bad mask, W = ceil(nx / 64) words a row: masks[plane][1 + RD_THR_MAX][ny][W], mask 0 the bad one.  A wave packs
//    RD_DM_PACK_ITEMS words, its lane 1 + t keeps the popcount of threshold t and adds it once to the plane's set size.
//  * k_dm_transform<RECORDS>: a workgroup owns a strip of SW adjacent columns (64; 32 where ny > 1024) of one threshold with all
//    ny rows of g resident in LDS as uint16, g(y, x) the distance to the nearest set bit of row y (0xFFFF: none), computed from the
//    mask words alone by clz / ctz on the word masked below and above the pixel's bit, walking over neighbouring words only where
//    the word is empty on that side.  Then a thread takes pixels of one column: d2 = min over y' of (y - y')^2 + g(y', x)^2, scanned
//    outward from y in both directions until k^2 >= best.  A plane narrower than SW / 2 is padded to the next power of two and
//    SW / that many planes of the pass lie side by side in the strip (a collage), so that nd 16 fills a wave with four planes.
//    An empty set skips both passes.  RECORDS = false writes D as uint16 (the observation's maps).  RECORDS = true keeps D(x, A) in
//    the register, reads D(x, B) and the observation at the same pixel and sums the twelve fields of the record over the thread's
//    pixels; a segment of lanes (a plane's share of the wave) is reduced by xor shuffles, its first lane adds to the workgroup's
//    record in LDS, and one 64-bit integer atomic per non-zero field goes to the record in memory.
// No floating-point atomics, no spin-waits, no grid sync.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_DM_MAXSIDE 2048               // ny, nx
#define RD_DM_MAXS 4096                  // members of one call
#define RD_DM_THREADS 256
#define RD_DM_NREC 12                    // 64-bit fields of a record
#define RD_DM_EMPTY 0xFFFFu              // D of an empty set, g of an empty row
#define RD_DM_INF 0x7FFFFFFFu            // d2 before any set pixel was seen
#define RD_DM_MAXPASS (1L << 20)         // planes of one pass
#define RD_DM_PACK_ITEMS 8               // row words a wave of k_dm_pack takes
#define RD_DM_CMIN 16                    // the cutoff in 1/16 pixel: 16 .. 65534
#define RD_DM_CMAX 65534

// the geometry of a call: the strips and the collage
struct rd_dm_geo {
  int ny, nx, W;                         // W: mask words a row
  int SW;                                // columns of a strip: 64, or 32 where ny > 1024 (ny SW uint16 stay within 128 KiB)
  int lseg;                              // log2 of a plane's share of the strip; 1 << lseg == SW without a collage
  int G;                                 // planes side by side in a strip: SW >> lseg
  int nstrips;                           // strips of a plane (1 in a collage)
};

inline rd_dm_geo rd_dm_geometry(long ny, long nx) {
  rd_dm_geo g;
  g.ny = (int)ny, g.nx = (int)nx, g.W = (int)((nx + 63) / 64);
  g.SW = ny > 1024 ? 32 : 64;
  int l = 0;
  while ((1 << l) < nx && (1 << l) < g.SW) ++l;
  g.lseg = l, g.G = g.SW >> l;
  g.nstrips = (int)((nx + g.SW - 1) / g.SW);
  return g;
}

// bytes of the workspace one plane takes: the 1 + RD_THR_MAX masks and the RD_THR_MAX set sizes
inline long rd_dm_plane_bytes(long ny, long nx) { return (1 + RD_THR_MAX) * ny * ((nx + 63) / 64) * 8 + RD_THR_MAX * 8; }
inline size_t rd_dm_lds_bytes(const rd_dm_geo& g) { return (size_t)g.ny * g.SW * sizeof(unsigned short); }

__device__ __forceinline__ unsigned long long rd_dm_shfl_xor64(unsigned long long v, int k) {
  const unsigned lo = __shfl_xor((unsigned)v, k), hi = __shfl_xor((unsigned)(v >> 32), k);
  return ((unsigned long long)hi << 32) | lo;
}

// grid (planes of the pass, chunks of 4 RD_DM_PACK_ITEMS row words).  Plane q0 + blockIdx.x of the array lies at
// x + (q / per_outer) * outer_stride + (q % per_outer) * ny nx: (24, day_stride) for days, (n_days 24, member_stride) for members.
// sizes[blockIdx.x * T + t] (zeroed by the caller) receives the set sizes
__global__ void __launch_bounds__(RD_DM_THREADS)
k_dm_pack(const float* __restrict__ x, long outer_stride, long per_outer, long q0, int ny, int nx, int W, rd_thr thr, int T,
          unsigned long long* __restrict__ masks, unsigned long long* __restrict__ sizes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long q = q0 + blockIdx.x, plane = (long)ny * nx;
  const float* src = x + (q / per_outer) * outer_stride + (q % per_outer) * plane;
  unsigned long long* out = masks + (long)blockIdx.x * (1 + RD_THR_MAX) * ny * W;
  const int items = ny * W, i0 = ((int)blockIdx.y * 4 + wave) * RD_DM_PACK_ITEMS;
  unsigned count = 0;                                                         // lane 1 + t: the events of threshold t
  for (int i = i0; i < min(i0 + RD_DM_PACK_ITEMS, items); ++i) {
    const int y = i / W, px = (i % W) * 64 + lane;
    const bool in = px < nx;
    const float v = in ? src[(long)y * nx + px] : 0.0f;
    unsigned long long mine = __ballot(in && rd_nonfinite(v));
#pragma unroll
    for (int t = 0; t < RD_THR_MAX; ++t)
      if (t < T) {
        const unsigned long long e = __ballot(in && !rd_nonfinite(v) && v > thr.v[t]);
        mine = lane == t + 1 ? e : mine;
      }
    if (lane <= T) out[(long)lane * items + i] = mine;
    if (lane >= 1) count += (unsigned)__popcll(mine);
  }
  if (lane >= 1 && lane <= T && count) atomicAdd(&sizes[(long)blockIdx.x * T + lane - 1], (unsigned long long)count);
}

// the distance from column x to the nearest set bit of a row of W words, RD_DM_EMPTY when the row has none
__device__ __forceinline__ unsigned rd_dm_row_dist(const unsigned long long* __restrict__ row, int W, int x) {
  const int w = x >> 6, b = x & 63;
  const unsigned long long cur = row[w];
  unsigned best = RD_DM_EMPTY;
  const unsigned long long lo = cur & (~0ull >> (63 - b));                    // the bits at or below b
  if (lo) {
    best = (unsigned)(b - (63 - __clzll((long long)lo)));
  } else {
    for (int k = w - 1; k >= 0; --k) {
      const unsigned long long v = row[k];
      if (v) {
        best = (unsigned)(x - (k * 64 + 63 - __clzll((long long)v)));
        break;
      }
    }
  }
  if (best == 0) return 0;
  const unsigned long long hi = cur & (~0ull << b);                           // the bits at or above b
  if (hi) {
    best = min(best, (unsigned)(__builtin_ctzll(hi) - b));
  } else {
    for (int k = w + 1; k < W; ++k) {
      const unsigned long long v = row[k];
      if (v) {
        best = min(best, (unsigned)(k * 64 + __builtin_ctzll(v) - x));
        break;
      }
    }
  }
  return best;
}

// grid (plane groups of the pass * strips, T).  Plane q0 + p of the array is plane p of the pass, p < P; its masks and sizes as
// k_dm_pack left them.  RECORDS = false: maps_out [plane of the array][T][ny][nx] uint16.  RECORDS = true: plane q of the members
// is compared with plane q % per_outer of obs (dense) and of obs_maps; records [q][T][RD_DM_NREC], zeroed by the caller
template <bool RECORDS>
__global__ void __launch_bounds__(RD_DM_THREADS)
k_dm_transform(rd_dm_geo geo, long q0, int P, int T, const unsigned long long* __restrict__ masks,
               const unsigned long long* __restrict__ sizes, unsigned short* __restrict__ maps_out, const float* __restrict__ obs,
               const unsigned short* __restrict__ obs_maps, long per_outer, rd_thr thr, int cutoff,
               unsigned long long* __restrict__ records) {
  extern __shared__ unsigned short rd_dm_g[];                                 // [ny][SW]
  __shared__ unsigned long long acc[64][RD_DM_NREC];                          // the records of the strip's planes
  const int tid = threadIdx.x, ny = geo.ny, nx = geo.nx, W = geo.W, SW = geo.SW;
  const int t = blockIdx.y;
  const int strip = (int)(blockIdx.x % geo.nstrips);
  const long group = blockIdx.x / geo.nstrips;
  const int c = tid % SW, r0 = tid / SW, RG = RD_DM_THREADS / SW;            // this thread's column of the strip and its rows
  const int segw = 1 << geo.lseg, pj = c >> geo.lseg;
  const int px = strip * SW + (c & (segw - 1));
  const long p = group * geo.G + pj;                                          // the plane of the pass
  const bool in = px < nx && p < P;
  if (RECORDS)
    for (int i = tid; i < 64 * RD_DM_NREC; i += RD_DM_THREADS) (&acc[0][0])[i] = 0ull;
  const long items = (long)ny * W;
  const unsigned long long* mp = masks + (in ? p : 0) * (1 + RD_THR_MAX) * items;
  const bool empty = in && sizes[p * T + t] == 0ull;
  const bool scan = in && !empty;

  if (scan) {
    const unsigned long long* ev = mp + (1 + t) * items;
    for (int y = r0; y < ny; y += RG) rd_dm_g[y * SW + c] = (unsigned short)rd_dm_row_dist(ev + (long)y * W, W, px);
  }
  __syncthreads();

  // the fields of this thread's pixels
  unsigned n_valid = 0, nA = 0, nB = 0, nAB = 0, maxBA = 0, maxAB = 0, maxW = 0, flags = 0;
  unsigned long long sumBA = 0, sumAB = 0, sum1 = 0, sum2 = 0;
  const long plane = (long)ny * nx;
  if (in) {
    const long q = q0 + p, r = q % per_outer;
    for (int y = r0; y < ny; y += RG) {
      unsigned D = RD_DM_EMPTY;
      if (scan) {
        const unsigned gy = rd_dm_g[y * SW + c];
        unsigned best = gy == RD_DM_EMPTY ? RD_DM_INF : gy * gy;
        const int kmax = max(y, ny - 1 - y);
        for (int k = 1; k <= kmax && (unsigned)(k * k) < best; ++k) {
          if (y - k >= 0) {
            const unsigned gg = rd_dm_g[(y - k) * SW + c];
            best = min(best, gg == RD_DM_EMPTY ? RD_DM_INF : (unsigned)(k * k) + gg * gg);
          }
          if (y + k < ny) {
            const unsigned gg = rd_dm_g[(y + k) * SW + c];
            best = min(best, gg == RD_DM_EMPTY ? RD_DM_INF : (unsigned)(k * k) + gg * gg);
          }
        }
        D = (unsigned)__dsqrt_rn((double)(best << 8));                        // isqrt(256 d2): exact, see the head of the file
      }
      if (!RECORDS) {
        maps_out[((q * T + t) * ny + y) * (long)nx + px] = (unsigned short)D;
      } else {
        const float o = obs[r * plane + (long)y * nx + px];
        const unsigned DB = obs_maps[((r * T + t) * ny + y) * (long)nx + px];
        const bool badA = (mp[(long)y * W + (px >> 6)] >> (px & 63)) & 1ull, badO = rd_nonfinite(o);
        const bool inA = D == 0, inB = !badO && o > thr.v[t], valid = !badA && !badO;
        const bool emptyB = DB == RD_DM_EMPTY;
        flags |= (unsigned)(badA != badO) | (empty ? 2u : 0u) | (emptyB ? 4u : 0u);
        if (valid) {
          n_valid += 1, nA += inA, nB += inB, nAB += inA && inB;
          if (inB && !empty) sumBA += D, maxBA = max(maxBA, D);
          if (inA && !emptyB) sumAB += DB, maxAB = max(maxAB, DB);
          const int wA = (int)min(D, (unsigned)cutoff), wB = (int)min(DB, (unsigned)cutoff);
          const unsigned d = (unsigned)abs(wA - wB);
          sum1 += d, sum2 += (unsigned long long)d * d, maxW = max(maxW, d);
        }
      }
    }
  }
  if (!RECORDS) return;

  // a plane's lanes of the wave -> its first lane -> the workgroup's record
  unsigned long long cnt = n_valid | ((unsigned long long)nA << 16) | ((unsigned long long)nB << 32) | ((unsigned long long)nAB << 48);
  const int red = geo.G == 1 ? 64 : segw;                                     // (without a collage both halves of a wave are one plane's)
  for (int k = 1; k < red; k <<= 1) {
    cnt += rd_dm_shfl_xor64(cnt, k);
    sumBA += rd_dm_shfl_xor64(sumBA, k), sumAB += rd_dm_shfl_xor64(sumAB, k);
    sum1 += rd_dm_shfl_xor64(sum1, k), sum2 += rd_dm_shfl_xor64(sum2, k);
    maxBA = max(maxBA, (unsigned)__shfl_xor(maxBA, k)), maxAB = max(maxAB, (unsigned)__shfl_xor(maxAB, k));
    maxW = max(maxW, (unsigned)__shfl_xor(maxW, k)), flags |= (unsigned)__shfl_xor(flags, k);
  }
  const bool leader = geo.G == 1 ? (tid & 63) == 0 : (c & (segw - 1)) == 0;
  if (leader && p < P) {
    unsigned long long* a = acc[pj];
    const unsigned long long add[RD_DM_NREC] = {cnt & 0xFFFFull, (cnt >> 16) & 0xFFFFull, (cnt >> 32) & 0xFFFFull, cnt >> 48, sumBA, sumAB,
                                                0, 0, sum1, sum2, 0, 0};
#pragma unroll
    for (int i = 0; i < RD_DM_NREC; ++i)
      if (add[i]) atomicAdd(&a[i], add[i]);
    if (maxBA) atomicMax(&a[6], (unsigned long long)maxBA);
    if (maxAB) atomicMax(&a[7], (unsigned long long)maxAB);
    if (maxW) atomicMax(&a[10], (unsigned long long)maxW);
    if (flags) atomicOr(&a[11], (unsigned long long)flags);
  }
  __syncthreads();
  for (int i = tid; i < geo.G * RD_DM_NREC; i += RD_DM_THREADS) {
    const int j = i / RD_DM_NREC, f = i % RD_DM_NREC;
    const long pp = group * geo.G + j;
    const unsigned long long v = acc[j][f];
    if (pp >= P || !v) continue;
    unsigned long long* dst = records + ((q0 + pp) * T + t) * RD_DM_NREC + f;
    if (f == 6 || f == 7 || f == 10) atomicMax(dst, v);
    else if (f == 11) atomicOr(dst, v);
    else atomicAdd(dst, v);
  }
}
