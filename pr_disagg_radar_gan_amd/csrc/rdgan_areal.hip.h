// Areal extremes of hourly fields: depth-area-duration.  For every day the largest accumulation over any k
// consecutive hours and any w x w box of pixels, for every window k and width w, and statistics of those maxima over the days.
// x [n][24][ny][nx] fp32 with a leading stride day_stride >= 24 ny nx.  q = (int) rintf(x * 1024) in units of 2^-10 mm; a
// pixel-hour is bad when x is NaN, +-inf, negative or >= 2048 (so q < 2^21, a 24-hour sum < 2^26, a box sum of 64 x 64 < 2^38).
// A(h0, y0, x0) is the sum of q over the hours h0 .. h0 + k - 1 and the pixels y0 .. y0 + w - 1, x0 .. x0 + w - 1, the box
// wholly inside the plane; a (window, box) with a bad pixel-hour is left out.  The day's key for (k, w) is the maximum of
// A 32 + (31 - h0): the largest A, and among equal ones the smallest h0; never 0, so 0 means "no admissible box".
//
// A pass holds D whole days in the workspace: keys [D][8][9] uint64, then S [D][24][plane] int32, then B [D][24][plane] uint8.
//  * k_areal_prefix: the only read of x.  One thread per pixel (or four) walks the 24 hours and stores the running sums
//    S[h] = q[0] + .. + q[h] (a bad hour adds 0) and the running counts B[h] of bad hours; it clears the keys of its day and
//    counts the bad pixel-hours.  The sum of a window is S[h0 + k - 1] - S[h0 - 1], and it is clean when B does not move.
//  * k_areal_boxes: one workgroup per (tile of 64 x 64 box corners, window, day).  For every h0 it loads the window sums of the
//    tile and a halo of wmax - 1 pixels into LDS as 64-bit words -- the sum in the low bits, 2^44 for a window with a bad hour --
//    and turns them into a summed-area table in place: one thread per row, then one thread per column.  A box of ANY width is
//    then four reads, I[y0 + w][x0 + w] - I[y0][x0 + w] - I[y0 + w][x0] + I[y0][x0], whose bits from 44 up count the bad pixels
//    of the box (at most 2^12) and whose low bits are A < 2^38: modulo 2^64 the four terms give exactly the sum over the box,
//    whatever the table's own size.  Every thread keeps the largest key of its corners per width over all h0; then one reduction
//    across the wave and one 64-bit atomicMax per wave and width.  Width 1 is always among the internal widths (slot 0): the
//    areal reduction factor needs the pixel maximum.
//  * k_areal_days: one workgroup column per (k, w), one thread per day: unpacks the key, classifies the day into an LDS copy
//    of the (k, w) record, which is merged into the state with 64-bit integer atomics, and writes depths_out.
// Kernel boundaries are the only ordering between the phases: no spin-wait, no grid sync, no floating-point atomic.  All global
// offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_AR_THREADS 256
#define RD_AR_TILE 64                    // box corners of a tile, each way
#define RD_AR_MAXK 8                     // windows
#define RD_AR_MAXW 8                     // widths the caller names
#define RD_AR_MAXWIDTH 64
#define RD_AR_MAXL 16                    // levels
#define RD_AR_SLOTS 9                    // internal widths: 1, then the caller's other widths
#define RD_AR_DAY_KEYS (RD_AR_MAXK * RD_AR_SLOTS)
#define RD_AR_MAXPASS 65535              // days of one pass: the grid's z
#define RD_AR_NARF 21                    // arf_hist[0 .. 20]
#define RD_AR_BADBIT 44                  // of an LDS word: bad windows are counted from this bit up
// the record of one (k, w), L levels: level_count[L + 1], then at L + 1 +
#define RD_AR_START 0                    // start_hour[24]
#define RD_AR_ARF 24                     // arf_hist[21]
#define RD_AR_SUM_A 45
#define RD_AR_SUM_A1 46
#define RD_AR_SUM_ALL 47
#define RD_AR_MAX_A 48
#define RD_AR_NDAYS 49
#define RD_AR_NVOID 50
#define RD_AR_NDRY 51
#define RD_AR_FIXED 52                   // words of a record besides level_count
#define RD_AR_MAXREC (RD_AR_MAXL + 1 + RD_AR_FIXED)

struct rd_ar_lists {
  int K, W, L, slots;                    // windows, widths, levels, internal widths
  int windows[RD_AR_MAXK];
  int widths[RD_AR_MAXW];
  int slot_width[RD_AR_SLOTS];           // slot 0 is width 1
  int slot_of[RD_AR_MAXW];               // the slot of the caller's width
  long long level_q[RD_AR_MAXL];         // rd_levels_q
};

__host__ __device__ inline long rd_ar_record(int L) { return L + 1 + RD_AR_FIXED; }
__host__ __device__ inline long rd_ar_state_count(int K, int W, int L) { return (long)K * W * rd_ar_record(L) + 2; }
// bytes of the workspace per day: the keys, 24 running sums and 24 running bad counts per pixel, rounded up to 8
__host__ __device__ inline long rd_ar_day_bytes(long plane) { return RD_AR_DAY_KEYS * 8 + (RD_HOURS * plane * 5 + 7) / 8 * 8; }
// the summed-area table of a tile: rows and row stride (in 8-byte words, odd: the lanes of the row scan fall on distinct banks)
__host__ __device__ inline int rd_ar_rows(int wmax) { return RD_AR_TILE + wmax; }
__host__ __device__ inline int rd_ar_stride(int wmax) { return (RD_AR_TILE + wmax) | 1; }
__host__ __device__ inline size_t rd_ar_lds_bytes(int wmax) { return (size_t)rd_ar_rows(wmax) * rd_ar_stride(wmax) * 8; }

// grid (ceil(plane / (V 256)), D).  V = 4 needs x 16-byte aligned and plane and day_stride multiples of 4.
template <int V>
__global__ void __launch_bounds__(RD_AR_THREADS)
k_areal_prefix(const float* __restrict__ x, long day_stride, long plane, long day0, unsigned long long* __restrict__ keys,
               int* __restrict__ S, unsigned char* __restrict__ B, unsigned long long* __restrict__ n_bad) {
  const long d = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x < RD_AR_DAY_KEYS) keys[d * RD_AR_DAY_KEYS + threadIdx.x] = 0ull;
  const long p = ((long)blockIdx.x * RD_AR_THREADS + threadIdx.x) * V;
  unsigned bad_here = 0;
  if (p < plane) {
    const float* xd = x + (day0 + d) * day_stride + p;
    int* Sd = S + d * RD_HOURS * plane + p;
    unsigned char* Bd = B + d * RD_HOURS * plane + p;
    int sum[V];
    unsigned bad[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sum[j] = 0, bad[j] = 0u;
#pragma unroll 8
    for (int h = 0; h < RD_HOURS; ++h) {
      float v[V];
      rd_load<V>(xd + h * plane, v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool b = rd_depth_bad(v[j]);
        sum[j] += b ? 0 : rd_depth_q(v[j]);
        bad[j] += b ? 1u : 0u;
      }
      if constexpr (V == 4) {
        *reinterpret_cast<int4*>(Sd + h * plane) = make_int4(sum[0], sum[1], sum[2], sum[3]);
        *reinterpret_cast<uchar4*>(Bd + h * plane) = make_uchar4((unsigned char)bad[0], (unsigned char)bad[1], (unsigned char)bad[2],
                                                                 (unsigned char)bad[3]);
      } else {
        Sd[h * plane] = sum[0];
        Bd[h * plane] = (unsigned char)bad[0];
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) bad_here += bad[j];
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) bad_here += __shfl_xor(bad_here, s);
  if ((threadIdx.x & 63) == 0 && bad_here) atomicAdd(n_bad, (unsigned long long)bad_here);
}

// grid (tiles_x tiles_y, K, D); dynamic LDS rd_ar_lds_bytes(wmax), wmax the largest internal width
__global__ void __launch_bounds__(RD_AR_THREADS)
k_areal_boxes(int ny, int nx, int tiles_x, rd_ar_lists lists, int wmax, const int* __restrict__ S, const unsigned char* __restrict__ B,
              unsigned long long* __restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long I[];
  const int tid = threadIdx.x;
  const int ty0 = (int)(blockIdx.x / tiles_x) * RD_AR_TILE, tx0 = (int)(blockIdx.x % tiles_x) * RD_AR_TILE;
  const int k = lists.windows[blockIdx.y];
  const long plane = (long)ny * nx, d = blockIdx.z;
  const int* Sd = S + d * RD_HOURS * plane;
  const unsigned char* Bd = B + d * RD_HOURS * plane;
  // the pixels of the plane the tile's boxes can cover, and the corners of the tile inside the plane
  const int ry = min(RD_AR_TILE + wmax - 1, ny - ty0), rx = min(RD_AR_TILE + wmax - 1, nx - tx0);
  const int cy = min(RD_AR_TILE, ny - ty0), cx = min(RD_AR_TILE, nx - tx0);
  const int LS = rd_ar_stride(wmax);
  // row 0 and column 0 of the table stay 0: no pass below writes them
  for (int i = tid; i <= rx; i += RD_AR_THREADS) I[i] = 0ull;
  for (int i = tid; i <= ry; i += RD_AR_THREADS) I[i * LS] = 0ull;
  unsigned long long best[RD_AR_SLOTS];
#pragma unroll
  for (int s = 0; s < RD_AR_SLOTS; ++s) best[s] = 0ull;
  for (int h0 = 0; h0 + k <= RD_HOURS; ++h0) {
    const int* hi = Sd + (long)(h0 + k - 1) * plane;
    const unsigned char* bhi = Bd + (long)(h0 + k - 1) * plane;
    const long lo = h0 ? -(long)k * plane : 0;                             // S[h0 - 1] from S[h0 + k - 1]; nothing before hour 0
    for (int i = tid; i < ry * rx; i += RD_AR_THREADS) {
      const int y = i / rx, c = i - y * rx;
      const long g = (long)(ty0 + y) * nx + tx0 + c;
      unsigned v = (unsigned)hi[g], b = bhi[g];
      if (h0) v -= (unsigned)hi[g + lo], b -= bhi[g + lo];
      I[(y + 1) * LS + c + 1] = (unsigned long long)v + ((unsigned long long)(b != 0u) << RD_AR_BADBIT);
    }
    __syncthreads();
    if (tid < ry) {
      unsigned long long run = 0ull, *row = I + (tid + 1) * LS;
#pragma unroll 8
      for (int c = 1; c <= rx; ++c) row[c] = run += row[c];
    }
    __syncthreads();
    if (tid < rx) {
      unsigned long long run = 0ull, *col = I + tid + 1;
#pragma unroll 8
      for (int y = 1; y <= ry; ++y) col[y * LS] = run += col[y * LS];
    }
    __syncthreads();
    const unsigned long long tag = 31ull - (unsigned)h0;
    for (int i = tid; i < cy * RD_AR_TILE; i += RD_AR_THREADS) {
      const int y = i / RD_AR_TILE, c = i % RD_AR_TILE;                    // a wave takes a row of corners
      if (c >= cx) continue;
      const unsigned long long* at = I + y * LS + c;
      const unsigned long long i00 = at[0];
#pragma unroll
      for (int s = 0; s < RD_AR_SLOTS; ++s) {
        if (s >= lists.slots) break;
        const int w = lists.slot_width[s];
        if (y + w > ry || c + w > rx) continue;                            // the box leaves the plane
        const unsigned long long a = at[w * LS + w] - at[w] - at[w * LS] + i00;
        const unsigned long long key = (a << 5) + tag;
        if (!(a >> RD_AR_BADBIT) && key > best[s]) best[s] = key;
      }
    }
    __syncthreads();
  }
  unsigned long long* out = keys + d * RD_AR_DAY_KEYS + (long)blockIdx.y * RD_AR_SLOTS;
#pragma unroll
  for (int s = 0; s < RD_AR_SLOTS; ++s) {
    if (s >= lists.slots) break;
    unsigned long long m = best[s];
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
      const unsigned long long o = __shfl_xor(m, j);
      m = o > m ? o : m;
    }
    if ((tid & 63) == 0 && m) atomicMax(&out[s], m);
  }
}

// grid (ceil(D / 256), K W); counts: the whole state; depths: null, or the map of the whole input, day0 the first day of the pass
__global__ void __launch_bounds__(RD_AR_THREADS)
k_areal_days(int D, long day0, rd_ar_lists lists, const unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts,
             long long* __restrict__ depths) {
  __shared__ unsigned long long tab[RD_AR_MAXREC];
  const int tid = threadIdx.x, L = lists.L, rec = (int)rd_ar_record(L);
  for (int i = tid; i < rec; i += RD_AR_THREADS) tab[i] = 0ull;
  __syncthreads();
  const int ki = blockIdx.y / lists.W, wi = blockIdx.y % lists.W;
  const int d = blockIdx.x * RD_AR_THREADS + tid;
  unsigned long long* fixed = tab + L + 1;
  if (d < D) {
    const unsigned long long* day = keys + (long)d * RD_AR_DAY_KEYS + ki * RD_AR_SLOTS;
    const unsigned long long key = day[lists.slot_of[wi]], key1 = day[0];
    long long depth = -1;
    if (!key) {
      atomicAdd(&fixed[RD_AR_NVOID], 1ull);
    } else {
      const unsigned long long A = key >> 5, A1 = key1 >> 5;               // (a clean box of any width holds a clean pixel)
      const unsigned long long w2 = (unsigned long long)lists.widths[wi] * lists.widths[wi];
      depth = (long long)A;
      int b = 0;
      for (int l = 0; l < L; ++l) b += A >= (unsigned long long)lists.level_q[l] * w2;
      atomicAdd(&tab[b], 1ull);
      atomicAdd(&fixed[RD_AR_START + 31 - (int)(key & 31)], 1ull);
      atomicAdd(&fixed[RD_AR_SUM_ALL], A);
      atomicMax(&fixed[RD_AR_MAX_A], A);
      atomicAdd(&fixed[RD_AR_NDAYS], 1ull);
      if (A1) {
        const unsigned long long r = 20ull * A / (w2 * A1);
        atomicAdd(&fixed[RD_AR_ARF + (r < 20ull ? (int)r : 20)], 1ull);
        atomicAdd(&fixed[RD_AR_SUM_A], A);
        atomicAdd(&fixed[RD_AR_SUM_A1], A1);
      } else {
        atomicAdd(&fixed[RD_AR_NDRY], 1ull);
      }
    }
    if (depths) depths[((day0 + d) * lists.K + ki) * lists.W + wi] = depth;
  }
  __syncthreads();
  unsigned long long* out = counts + (long)blockIdx.y * rec;
  for (int i = tid; i < rec; i += RD_AR_THREADS) {
    if (!tab[i]) continue;
    if (i == L + 1 + RD_AR_MAX_A) atomicMax(&out[i], tab[i]);
    else atomicAdd(&out[i], tab[i]);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) atomicAdd(&counts[(long)lists.K * lists.W * rec], (unsigned long long)D);
}
