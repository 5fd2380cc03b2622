// Space-time structure of hourly fields: the wet/dry agreement between hour h at pixel p and hour h + k at
// pixel p + d for every displacement |dy|, |dx| <= R, and for every pair of hours the displacement that best maps one wet mask
// onto the other.  x [n][24][ny][nx] fp32 with a leading stride day_stride >= 24 ny nx.  A pixel is wet for threshold t when
// x > thr[t] in fp32 and it is finite, bad when it is NaN or +-inf (never wet).  Hours pair inside a day only.
//
// The workspace holds, for the days of a pass, bit masks [day][24][1 + T][ny][W] of 64-bit words, W = ceil(nx / 64): bit b of word
// w of a row is pixel 64 w + b; mask 0 is "not bad", mask 1 + t is "wet at threshold t"; the bits past nx are zero.
//
//  * k_st_pack streams the input once.  V = 1: a wave takes 64 adjacent pixels of a row, the ballot of a compare IS the word.
//    V = 4 (16-byte loads: x 16-byte aligned, nx and day_stride multiples of 4): a lane holds 4 adjacent pixels, its 4 compares
//    are a nibble, three shuffles join the nibbles of 8 lanes and every eighth lane stores 32 bits.  Bad pixels are counted here,
//    once, and so are the days.
//  * k_st_correlate: one workgroup per (day, lag k, group of RD_ST_HPB hours, threshold).  It walks the plane pair (h, h + k) in
//    tiles of bh rows x cw words: the tile of A (not-bad and wet words) and the tile of B with R halo rows and one halo word on
//    each side, zero outside the plane, lie in LDS.  A thread owns a (displacement, row slice); the row of B shifted by dx is a
//    funnel shift of two neighbouring words, and every count is a sum of popcounts of the AND (the pooled counts) or of the XOR
//    under the core's column mask (dist) of whole words.  Zero words outside the plane restrict the pooled counts to P(d) by
//    themselves.  Counts are added per displacement to a 32-bit LDS table (a plane has at most 2^24 pixels, a workgroup at most 6
//    planes); the pair's argmin is one 64-bit integer min over the key (dist, dy^2 + dx^2, dy + R, dx + R); the pooled counts
//    are merged into the state once per workgroup with 64-bit integer atomics.  pairs[k][d] is formed by the workgroups of
//    threshold 0 only.
// No floating-point atomics, no spin-waits, no grid sync: the kernel boundary between the two is the only ordering.  All global
// offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_ST_MAXT RD_THR_MAX
#define RD_ST_MAXR 8
#define RD_ST_MAXK 6
#define RD_ST_THREADS 256
#define RD_ST_MAXPASS 65520              // planes of one pass: 2730 whole days
#define RD_ST_HPB 6                      // hours of one (day, k) a workgroup of k_st_correlate takes
#define RD_ST_GROUPS 4                   // 24 / RD_ST_HPB
#define RD_ST_MAXCW 8                    // words of a row a tile holds at most
#define RD_ST_LDS_WORDS 4096             // 64-bit words of LDS the four tile arrays share
#define RD_ST_MAXNS 16                   // row slices of a tile at most
#define RD_ST_PACK_MAXBLOCKS 4096

// the state for (T, R, K), D = (2R + 1)^2, d = (dy + R)(2R + 1) + dx + R: pairs[K + 1][D], then per threshold a block of
// rd_st_per_threshold words -- wet_first[K + 1][D], wet_second[K + 1][D], joint[K + 1][D], shift_hist[K][D] (lags 1 .. K),
// no_shift[K], dist_best[K], dist_zero[K] -- then n_days and n_bad_pixels
__host__ __device__ inline long rd_st_nd(int R) { return (long)(2 * R + 1) * (2 * R + 1); }
__host__ __device__ inline long rd_st_per_threshold(int R, int K) { return (3L * (K + 1) + K) * rd_st_nd(R) + 3L * K; }
__host__ __device__ inline long rd_st_thr_base(int R, int K, int t) { return (K + 1) * rd_st_nd(R) + t * rd_st_per_threshold(R, K); }
__host__ __device__ inline long rd_st_state_count(int T, int R, int K) { return rd_st_thr_base(R, K, T) + 2; }
// bytes of the masks of one plane
__host__ __device__ inline long rd_st_plane_bytes(long ny, long nx, int T) { return (long)(T + 1) * ny * ((nx + 63) / 64) * 8; }

// the tile of k_st_correlate: cw words wide, and the tallest bh with 2 bh cw + 2 (bh + 2R)(cw + 2) <= RD_ST_LDS_WORDS, the bands
// then evened out over the rows
inline void rd_st_tile(long ny, long nx, int R, int* cw, int* bh) {
  const long W = (nx + 63) / 64;
  const int c = (int)(W < RD_ST_MAXCW ? W : RD_ST_MAXCW);
  const long bhmax = (RD_ST_LDS_WORDS - 4L * R * (c + 2)) / (4L * c + 4);
  const long bands = (ny + bhmax - 1) / bhmax;
  *cw = c;
  *bh = (int)((ny + bands - 1) / bands);
}
inline size_t rd_st_lds_bytes(int R, int cw, int bh) {
  return ((size_t)2 * bh * cw + (size_t)2 * (bh + 2 * R) * (cw + 2) + 1 + cw) * 8 + ((size_t)5 * rd_st_nd(R) + 2) * 4;
}
// row slices of a tile: the count in 1 .. min(16, bh) that leaves the fewest idle threads in the last round of D ns items
inline int rd_st_slices(int R, int bh) {
  const long D = rd_st_nd(R);
  int best = 1;
  double eff = 0.0;
  for (int ns = 1; ns <= RD_ST_MAXNS && ns <= bh; ++ns) {
    const long items = D * ns, rounds = (items + RD_ST_THREADS - 1) / RD_ST_THREADS;
    const double e = (double)items / (double)(rounds * RD_ST_THREADS);
    if (e > eff + 1e-9) {
      eff = e;
      best = ns;
    }
  }
  return best;
}

// the core's columns R <= x < nx - R among the 64 of word w
__device__ __forceinline__ unsigned long long rd_st_core_mask(int w, int nx, int R) {
  const int lo = R - 64 * w > 0 ? R - 64 * w : 0, hi = nx - R - 64 * w < 64 ? nx - R - 64 * w : 64;
  if (hi <= lo) return 0ull;
  const unsigned long long below_hi = hi == 64 ? ~0ull : (1ull << hi) - 1ull;
  return below_hi & ~((1ull << lo) - 1ull);
}

template <int V>
__global__ void __launch_bounds__(RD_ST_THREADS)
k_st_pack(const float* __restrict__ x, long day_stride, int ny, int nx, int W, long day0, long days, rd_thr thr, int T,
          unsigned long long* __restrict__ masks, unsigned long long* __restrict__ n_days, unsigned long long* __restrict__ bad_count) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * RD_ST_THREADS + threadIdx.x) >> 6, nwaves = (long)gridDim.x * (RD_ST_THREADS / 64);
  const long plane = (long)ny * nx;
  const int per_row = V == 4 ? (W + 3) / 4 : W;                          // items of a row: 256 or 64 pixels each
  const long items = days * RD_HOURS * ny * per_row;
  unsigned n_bad = 0;
  for (long it = wave; it < items; it += nwaves) {                        // (the same trip count in every lane of a wave)
    const int c = (int)(it % per_row);
    const long r = it / per_row;
    const int y = (int)(r % ny);
    const long pl = r / ny;                                               // the plane of the pass: day * 24 + hour
    const float* src = x + (day0 + pl / RD_HOURS) * day_stride + (pl % RD_HOURS) * plane + (long)y * nx;
    unsigned long long* row = masks + (pl * (T + 1) * ny + y) * W;        // mask m of this row lies m * ny * W words on
    const long mstride = (long)ny * W;
    if constexpr (V == 1) {
      const int px = c * 64 + lane;
      const bool in = px < nx;
      const float v = in ? src[px] : 0.0f;
      const bool bad = in && rd_nonfinite(v), ok = in && !bad;
      n_bad += bad;
      unsigned long long mine = __ballot(ok);                             // lane m keeps mask m
#pragma unroll
      for (int t = 0; t < RD_ST_MAXT; ++t)
        if (t < T) {
          const unsigned long long b = __ballot(ok && v > thr.v[t]);
          mine = lane == t + 1 ? b : mine;
        }
      if (lane <= T) row[lane * mstride + c] = mine;
    } else {
      const int px = c * 256 + 4 * lane;
      float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (px < nx) rd_load<4>(src + px, v);                            // (nx % 4 == 0: all four or none)
      bool ok[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool bad = px < nx && rd_nonfinite(v[j]);
        ok[j] = px < nx && !bad;
        n_bad += bad;
      }
      const bool store = (lane & 7) == 0 && px < W * 64;                  // 32 pixels: one 32-bit half of a word
      unsigned* row32 = reinterpret_cast<unsigned*>(row);
#pragma unroll
      for (int m = 0; m <= RD_ST_MAXT; ++m)
        if (m <= T) {
          unsigned nib = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) nib |= (unsigned)(ok[j] && (m == 0 || v[j] > thr.v[m ? m - 1 : 0])) << j;
          nib |= __shfl_down(nib, 1) << 4;
          nib |= __shfl_down(nib, 2) << 8;
          nib |= __shfl_down(nib, 4) << 16;
          if (store) row32[m * mstride * 2 + c * 8 + (lane >> 3)] = nib;
        }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) n_bad += __shfl_xor(n_bad, s);
  if (lane == 0 && n_bad) atomicAdd(bad_count, (unsigned long long)n_bad);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(n_days, (unsigned long long)days);
}

// grid (days of the pass x (K + 1) x RD_ST_GROUPS, T); masks: of the pass; counts: the state
__global__ void __launch_bounds__(RD_ST_THREADS)
k_st_correlate(const unsigned long long* __restrict__ masks, int ny, int nx, int W, int T, int R, int K, int cw, int bh, int ns,
               unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned long long rd_st_lds[];
  const int side = 2 * R + 1, D = side * side, bwid = cw + 2, brows = bh + 2 * R;
  unsigned long long* a_nb = rd_st_lds;                                    // [bh][cw]
  unsigned long long* a_w = a_nb + bh * cw;                                // [bh][cw]
  unsigned long long* b_nb = a_w + bh * cw;                                // [bh + 2R][cw + 2]
  unsigned long long* b_w = b_nb + brows * bwid;                           // [bh + 2R][cw + 2]
  unsigned long long* key = b_w + brows * bwid;                            // the pair's smallest (dist, dy^2 + dx^2, dy + R, dx + R)
  unsigned long long* cmask = key + 1;                                     // [cw]: the core's columns in the words of the tile
  unsigned* acc = reinterpret_cast<unsigned*>(cmask + cw);                 // [5][D]: pairs, wet_first, wet_second, joint; dist
  unsigned* cnt = acc + 5 * D;                                             // wet pixels of A in the core, of B in the plane

  const int tid = threadIdx.x, lane = tid & 63;
  const int t = blockIdx.y, g = blockIdx.x % RD_ST_GROUPS, k = (blockIdx.x / RD_ST_GROUPS) % (K + 1);
  const long day = blockIdx.x / (RD_ST_GROUPS * (K + 1));
  const int h0 = g * RD_ST_HPB, h1 = h0 + RD_ST_HPB < RD_HOURS - k ? h0 + RD_ST_HPB : RD_HOURS - k;
  const bool first = t == 0;
  const long mplane = (long)ny * W;
  unsigned long long* tb = counts + rd_st_thr_base(R, K, t);
  for (int i = tid; i < 4 * D; i += RD_ST_THREADS) acc[i] = 0u;
  const int rs = (bh + ns - 1) / ns;                                       // rows of a slice

  for (int h = h0; h < h1; ++h) {
    for (int i = tid; i < D; i += RD_ST_THREADS) acc[4 * D + i] = 0u;
    if (tid < 2) cnt[tid] = 0u;
    if (tid == 2) *key = ~0ull;
    const unsigned long long* ga = masks + (day * RD_HOURS + h) * (T + 1) * mplane;
    const unsigned long long* gb = masks + (day * RD_HOURS + h + k) * (T + 1) * mplane;
    for (int y0 = 0; y0 < ny; y0 += bh)
      for (int w0 = 0; w0 < W; w0 += cw) {
        __syncthreads();                                                   // the tile before this one is done with, the zeros are written
        unsigned ca = 0, cb = 0;
        for (int i = tid; i < bh * cw; i += RD_ST_THREADS) {
          const int y = y0 + i / cw, w = w0 + i % cw;
          const bool in = y < ny && w < W;
          const unsigned long long nbv = in ? ga[(long)y * W + w] : 0ull, wv = in ? ga[(1 + t) * mplane + (long)y * W + w] : 0ull;
          a_nb[i] = nbv;
          a_w[i] = wv;
          if (in && y >= R && y < ny - R) ca += (unsigned)__popcll(wv & rd_st_core_mask(w, nx, R));
        }
        for (int i = tid; i < brows * bwid; i += RD_ST_THREADS) {
          const int r = i / bwid, c = i % bwid, y = y0 - R + r, w = w0 - 1 + c;
          const bool in = y >= 0 && y < ny && w >= 0 && w < W;
          const unsigned long long nbv = in ? gb[(long)y * W + w] : 0ull, wv = in ? gb[(1 + t) * mplane + (long)y * W + w] : 0ull;
          b_nb[i] = nbv;
          b_w[i] = wv;
          if (r >= R && r < R + bh && c >= 1 && c <= cw) cb += (unsigned)__popcll(wv);          // (every word of B once)
        }
        if (tid < cw) cmask[tid] = rd_st_core_mask(w0 + tid, nx, R);
        if (ca) atomicAdd(&cnt[0], ca);
        if (cb) atomicAdd(&cnt[1], cb);
        __syncthreads();

        const int cwe = W - w0 < cw ? W - w0 : cw, rows = ny - y0 < bh ? ny - y0 : bh;
        for (int item = tid; item < D * ns; item += RD_ST_THREADS) {
          const int d = item % D, s = item / D, dy = d / side - R, dx = d % side - R;
          const int r0 = s * rs, r1 = r0 + rs < rows ? r0 + rs : rows;
          // B shifted by dx: bit b of the word is B's pixel 64 w + b + dx, from words (w, w + 1) or (w - 1, w)
          const int sh = dx >= 0 ? dx : 64 + dx, cofs = dx >= 0 ? 1 : 0;
          unsigned pa = 0, wf = 0, ws = 0, jn = 0, di = 0;
          for (int r = r0; r < r1; ++r) {
            const int y = y0 + r;
            const bool core = k > 0 && y >= R && y < ny - R;
            const unsigned long long* an = a_nb + r * cw;
            const unsigned long long* aw = a_w + r * cw;
            const int br = (r + dy + R) * bwid + cofs;
            unsigned long long lnb = b_nb[br], lw = b_w[br];
            for (int c = 0; c < cwe; ++c) {
              const unsigned long long hnb = b_nb[br + c + 1], hw = b_w[br + c + 1];
              const unsigned long long snb = (lnb >> sh) | ((hnb << 1) << (63 - sh)), sw = (lw >> sh) | ((hw << 1) << (63 - sh));
              const unsigned long long anb = an[c], awv = aw[c];
              if (first) pa += (unsigned)__popcll(anb & snb);
              wf += (unsigned)__popcll(awv & snb);
              ws += (unsigned)__popcll(anb & sw);
              jn += (unsigned)__popcll(awv & sw);
              if (core) di += (unsigned)__popcll((awv ^ sw) & cmask[c]);
              lnb = hnb;
              lw = hw;
            }
          }
          if (pa) atomicAdd(&acc[d], pa);
          if (wf) atomicAdd(&acc[D + d], wf);
          if (ws) atomicAdd(&acc[2 * D + d], ws);
          if (jn) atomicAdd(&acc[3 * D + d], jn);
          if (di) atomicAdd(&acc[4 * D + d], di);
        }
      }
    __syncthreads();
    if (k > 0) {                                                           // (the same in the whole workgroup)
      unsigned long long best = ~0ull;
      for (int d = tid; d < D; d += RD_ST_THREADS) {
        const int dy = d / side - R, dx = d % side - R;
        const unsigned long long q = ((unsigned long long)acc[4 * D + d] << 18) | ((unsigned long long)(dy * dy + dx * dx) << 10) |
                                     ((unsigned long long)(dy + R) << 5) | (unsigned long long)(dx + R);
        best = q < best ? q : best;
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(best, s);
        best = o < best ? o : best;
      }
      if (lane == 0) atomicMin(key, best);
      __syncthreads();
      if (tid == 0) {
        if (cnt[0] == 0u || cnt[1] == 0u) {
          atomicAdd(&tb[(3L * (K + 1) + K) * D + (k - 1)], 1ull);         // no_shift
        } else {
          const unsigned long long q = *key;
          const int dstar = (int)((q >> 5) & 31) * side + (int)(q & 31);
          atomicAdd(&tb[3L * (K + 1) * D + (long)(k - 1) * D + dstar], 1ull);
          if (q >> 18) atomicAdd(&tb[(3L * (K + 1) + K) * D + K + (k - 1)], q >> 18);
          const unsigned dz = acc[4 * D + R * side + R];
          if (dz) atomicAdd(&tb[(3L * (K + 1) + K) * D + 2 * K + (k - 1)], (unsigned long long)dz);
        }
      }
      __syncthreads();                                                     // key and dist are read before the next hour resets them
    }
  }
  __syncthreads();
  for (int d = tid; d < D; d += RD_ST_THREADS) {
    if (first && acc[d]) atomicAdd(&counts[(long)k * D + d], (unsigned long long)acc[d]);
    if (acc[D + d]) atomicAdd(&tb[(long)k * D + d], (unsigned long long)acc[D + d]);
    if (acc[2 * D + d]) atomicAdd(&tb[(long)(K + 1 + k) * D + d], (unsigned long long)acc[2 * D + d]);
    if (acc[3 * D + d]) atomicAdd(&tb[(long)(2 * (K + 1) + k) * D + d], (unsigned long long)acc[3 * D + d]);
  }
}
