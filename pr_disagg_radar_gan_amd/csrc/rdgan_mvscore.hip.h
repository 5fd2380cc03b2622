// Joint-field scores of ensembles of hourly days: the energy score's two sums of Euclidean distances and the
// variogram score's squared differences per displacement.  A day is d = 24 ny nx components; x [m][24][ny][nx] fp32 is an ensemble
// (finite values), y [24][ny][nx] the observed day, a NaN of y leaves its position out of every sum of that day.
//
//  * k_mv_valid counts the valid positions of every observed day (fixed tree, no atomics); a day without one gets NaN outputs.
//  * k_mv_energy: the rows of a day are its m members and, as row m, the observation.  A workgroup owns a 64 x 64 tile (ti <= tj) of
//    the symmetric distance matrix and streams the d components through LDS in chunks of 32, two buffers, the next chunk fetched to
//    registers while the current one is used.  A thread keeps rows ty + 16 a and columns tx + 16 b (a, b = 0 .. 3) -- with the LDS
//    row stride of 36 floats the 16 column reads of a wave fall on 16 different 16-byte slots -- as 16 fp64 sums of squared fp64
//    differences: one v_add_f64 and one v_fma_f64 per pair-component.  A masked position is staged as 0 in every row, so its
//    difference is exactly 0; equal members give exactly 0.  At the end: square roots, i >= j dropped on diagonal tiles, two sums
//    (distances to the observation, distances among members) reduced in a fixed tree and written to the tile's slot.
//    COLS = true is the shared-ensemble form's second launch: the columns are 64 observed days, each with its own mask, so the
//    difference is fma(a, f, -b') with f = 0 or 1 and b' = 0 at a NaN (the same rounding as a - b); a slot holds, per day, the sum
//    over the tile's members.
//  * k_mv_energy_reduce adds the slots of a day in slot order.
//  * k_mv_variogram: a workgroup owns (day, lag l, hour h, group of 16 displacements, 16 x 16 tile of anchors).  Per member, in
//    order, the tile of hour h + l with a halo of `radius` lies in LDS (two buffers, one barrier per member), the anchor in a
//    register; a thread adds |a - b|^p (fp32) for its anchor and the group's displacements into 16 fp64 registers.  MODE 0 then
//    forms (o - mean)^2 where both ends are valid and reduces sq and count per displacement in a fixed tree into the unit's slot;
//    MODE 1 writes the means to a table instead (the shared ensemble, once); MODE 2 starts from that table (one cheap pass per
//    observed day).  The three share every line that rounds, so the shared form equals the per-day form bit for bit.
//  * k_mv_variogram_reduce adds the slots of (day, lag, displacement) in order of hour and tile.
// No floating-point atomics, no spin-waits.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_MV_MAXM 8192                  // members (RD_CRPS_MAXN)
#define RD_MV_MAXDAYS (1L << 20)         // observed days of a call
#define RD_MV_MAXR 4
#define RD_MV_MAXLAG 3
#define RD_MV_THREADS 256
#define RD_MV_TILE 64                    // rows and columns of an energy tile
#define RD_MV_CHUNK 32                   // components of a chunk
#define RD_MV_LDK 36                     // floats of a panel row in LDS
#define RD_MV_VT 16                      // the anchors of a variogram tile are RD_MV_VT x RD_MV_VT
#define RD_MV_VG 16                      // displacements of a group
#define RD_MV_MAXBLOCKS 2147483647L

__host__ __device__ inline long rd_mv_tiles(long rows) { return (rows + RD_MV_TILE - 1) / RD_MV_TILE; }
__host__ __device__ inline long rd_mv_tile_pairs(long T) { return T * (T + 1) / 2; }
// the energy workspace, in 8-byte words: nvalid [D]; per-day form: slots [D][NT(m + 1)][2]; shared form: member slots
// [1 + D][NT(m)] (block 0: no mask; block 1 + d: the mask of day d, written only when that day has a NaN) and observation slots
// [T(m)][64 T(D)]
__host__ __device__ inline long rd_mv_energy_words(long m, long D, int shared) {
  if (!shared) return D + D * rd_mv_tile_pairs(rd_mv_tiles(m + 1)) * 2;
  return D + (1 + D) * rd_mv_tile_pairs(rd_mv_tiles(m)) + rd_mv_tiles(m) * rd_mv_tiles(D) * RD_MV_TILE;
}

// displacements of lag l in the flat order (di + R)(2R + 1) + dj + R: all of them for l > 0, those behind the centre for l = 0
__host__ __device__ inline int rd_mv_side(int R) { return 2 * R + 1; }
__host__ __device__ inline int rd_mv_first(int R, int l) { return l > 0 ? 0 : R * rd_mv_side(R) + R + 1; }
__host__ __device__ inline int rd_mv_count(int R, int l) { return rd_mv_side(R) * rd_mv_side(R) - rd_mv_first(R, l); }
__host__ __device__ inline int rd_mv_groups(int R, int l) { return (rd_mv_count(R, l) + RD_MV_VG - 1) / RD_MV_VG; }
__host__ __device__ inline long rd_mv_vtiles(long ny, long nx) { return ((ny + RD_MV_VT - 1) / RD_MV_VT) * ((nx + RD_MV_VT - 1) / RD_MV_VT); }
// units (workgroups) of a day: lag-major, then hour, group, tile
__host__ __device__ inline long rd_mv_unit_base(long ny, long nx, int R, int l) {
  long u = 0;
  for (int k = 0; k < l; ++k) u += (long)(RD_HOURS - k) * rd_mv_groups(R, k) * rd_mv_vtiles(ny, nx);
  return u;
}
__host__ __device__ inline long rd_mv_units(long ny, long nx, int R, int L) { return rd_mv_unit_base(ny, nx, R, L + 1); }
// the variogram workspace, in 8-byte words: nvalid [D]; slots [D][units][16][2]; shared form: and the table of means
// [units][16][256]
__host__ __device__ inline long rd_mv_variogram_words(long D, long ny, long nx, int R, int L, int shared) {
  const long U = rd_mv_units(ny, nx, R, L);
  return D + D * U * RD_MV_VG * 2 + (shared ? U * RD_MV_VG * RD_MV_THREADS : 0);
}

__device__ __forceinline__ bool rd_mv_nan(float v) { return v != v; }

// ---- valid positions of a day: one workgroup per day
__global__ void __launch_bounds__(RD_MV_THREADS)
k_mv_valid(const float* __restrict__ obs, long P, long long* __restrict__ nvalid) {
  __shared__ long long part[RD_MV_THREADS];
  const float* y = obs + (long)blockIdx.x * P;
  long long n = 0;
  for (long p = threadIdx.x; p < P; p += RD_MV_THREADS) n += !rd_mv_nan(y[p]);
  part[threadIdx.x] = n;
  __syncthreads();
  for (int s = RD_MV_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) nvalid[blockIdx.x] = part[0];
}

// ---- energy score
// One panel element per (row, component) a thread stages: 64 rows x 32 components = 2048, 8 per thread; thread t takes component
// t % 32 of rows t / 32 + 8 q: a wave reads two runs of 32 adjacent floats.
#define RD_MV_STAGE 8

// COLS = false: grid = days x NT tiles.  rows r < m: ens + (day * ens_day_stride) + r P; row m (with_obs): obs + day P.
//   The NaNs of obs[day] mask every row.  shared_members (the shared form's member launch, with_obs = 0, grid = (1 + days) x NT):
//   block 0 has no mask, block 1 + d has the mask of day d and returns at once unless 0 < nvalid[d] < P.
// COLS = true: grid = T(m) x T(D); the columns are the observed days.
template <bool COLS>
__global__ void __launch_bounds__(RD_MV_THREADS)
k_mv_energy(const float* __restrict__ ens, long ens_day_stride, const float* __restrict__ obs, int m, long n_days, long P, int with_obs,
            int shared_members, const long long* __restrict__ nvalid, double* __restrict__ slots) {
  constexpr int NP = COLS ? 3 : 2;
  __shared__ __attribute__((aligned(16))) float panel[2][NP][RD_MV_TILE * RD_MV_LDK];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int sc = tid & 31, sr = tid >> 5;                                  // the staged component and first row

  long day = 0;
  int ti, tj, T;
  const float* mask = nullptr;                                             // the observed day whose NaNs mask every row
  double* slot;
  if constexpr (COLS) {
    T = (int)rd_mv_tiles(m);
    const long TD = rd_mv_tiles(n_days);
    ti = (int)(blockIdx.x / TD);
    tj = (int)(blockIdx.x % TD);
    slot = slots + ((long)ti * TD + tj) * RD_MV_TILE;
  } else {
    const int rows = m + (with_obs ? 1 : 0);
    T = (int)rd_mv_tiles(rows);
    const long NT = rd_mv_tile_pairs(T);
    const long blk = blockIdx.x / NT;
    long t = blockIdx.x % NT;
    if (shared_members) {
      if (blk > 0) {
        day = blk - 1;
        const long long nv = nvalid[day];
        if (nv == 0 || nv == P) return;                                    // block 0 serves this day, or nothing does
        mask = obs + day * P;
      }
    } else {
      day = blk;
      mask = obs + day * P;
    }
    ti = 0;
    while (t >= T - ti) {
      t -= T - ti;
      ++ti;
    }
    tj = ti + (int)t;
    slot = slots + (long)blockIdx.x * (with_obs ? 2 : 1);
  }

  // the rows this thread stages: pointers (null: a row behind the last one, staged as 0)
  const float* arow[RD_MV_STAGE];
  const float* brow[RD_MV_STAGE];
#pragma unroll
  for (int q = 0; q < RD_MV_STAGE; ++q) {
    const int r = sr + 8 * q;
    const long ia = (long)ti * RD_MV_TILE + r, ib = (long)tj * RD_MV_TILE + r;
    if constexpr (COLS) {
      arow[q] = ia < m ? ens + ia * P : nullptr;
      brow[q] = ib < n_days ? obs + ib * P : nullptr;
    } else {
      const float* e = ens + day * ens_day_stride;
      arow[q] = ia < m ? e + ia * P : (with_obs && ia == m ? obs + day * P : nullptr);
      brow[q] = ib < m ? e + ib * P : (with_obs && ib == m ? obs + day * P : nullptr);
    }
  }

  float sa[RD_MV_STAGE], sb[RD_MV_STAGE], sf[RD_MV_STAGE];
  auto fetch = [&](long c0) {
    const long p = c0 + sc;
    const bool in = p < P;
    bool keep = in;
    if constexpr (!COLS) {
      if (mask != nullptr && in) keep = !rd_mv_nan(mask[p]);
    }
#pragma unroll
    for (int q = 0; q < RD_MV_STAGE; ++q) {
      float a = 0.0f, b = 0.0f, f = 0.0f;
      if (keep && arow[q] != nullptr) a = arow[q][p];
      if (keep && brow[q] != nullptr) b = brow[q][p];
      if constexpr (COLS) {
        f = (keep && brow[q] != nullptr && !rd_mv_nan(b)) ? 1.0f : 0.0f;
        if (f == 0.0f) b = 0.0f;
      }
      sa[q] = a;
      sb[q] = b;
      sf[q] = f;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < RD_MV_STAGE; ++q) {
      const int at = (sr + 8 * q) * RD_MV_LDK + sc;
      panel[buf][0][at] = sa[q];
      panel[buf][1][at] = sb[q];
      if constexpr (COLS) panel[buf][2][at] = sf[q];
    }
  };

  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

  const long nchunks = (P + RD_MV_CHUNK - 1) / RD_MV_CHUNK;
  fetch(0);
  for (long ch = 0; ch < nchunks; ++ch) {
    const int buf = (int)(ch & 1);
    stage(buf);
    __syncthreads();                                                       // (the other buffer was last read before the barrier of chunk ch - 1)
    if (ch + 1 < nchunks) fetch((ch + 1) * RD_MV_CHUNK);
#pragma unroll 2
    for (int c4 = 0; c4 < RD_MV_CHUNK; c4 += 4) {
      float4 av[4], bv[4], fv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = *reinterpret_cast<const float4*>(&panel[buf][0][(ty + 16 * a) * RD_MV_LDK + c4]);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        bv[b] = *reinterpret_cast<const float4*>(&panel[buf][1][(tx + 16 * b) * RD_MV_LDK + c4]);
        if constexpr (COLS) fv[b] = *reinterpret_cast<const float4*>(&panel[buf][2][(tx + 16 * b) * RD_MV_LDK + c4]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double ad[4], bd[4], fd[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) ad[a] = (double)(reinterpret_cast<const float*>(&av[a])[c]);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          bd[b] = (double)(reinterpret_cast<const float*>(&bv[b])[c]);
          if constexpr (COLS) fd[b] = (double)(reinterpret_cast<const float*>(&fv[b])[c]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            double df;
            if constexpr (COLS)
              df = __fma_rn(ad[a], fd[b], -bd[b]);
            else
              df = __dsub_rn(ad[a], bd[b]);
            acc[a][b] = __fma_rn(df, df, acc[a][b]);
          }
      }
    }
  }
  __syncthreads();                                                         // the panels are done with: their LDS becomes the reduction's

  double* red = reinterpret_cast<double*>(&panel[0][0][0]);
  if constexpr (COLS) {
    // per column (day) the sum over this thread's rows, then over the 16 ty in order
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const long i = (long)ti * RD_MV_TILE + ty + 16 * a;
        s += i < m ? sqrt(acc[a][b]) : 0.0;
      }
      red[ty * RD_MV_TILE + tx + 16 * b] = s;
    }
    __syncthreads();
    if (tid < RD_MV_TILE) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += red[k * RD_MV_TILE + tid];
      slot[tid] = s;
    }
  } else {
    const int rows = m + (with_obs ? 1 : 0);
    double so = 0.0, sp = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const long i = (long)ti * RD_MV_TILE + ty + 16 * a, j = (long)tj * RD_MV_TILE + tx + 16 * b;
        if (i < j && j < rows) {
          const double dist = sqrt(acc[a][b]);
          if (with_obs && j == m)
            so += dist;
          else
            sp += dist;
        }
      }
    red[tid] = so;
    red[RD_MV_THREADS + tid] = sp;
    __syncthreads();
    for (int s = RD_MV_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        red[tid] += red[tid + s];
        red[RD_MV_THREADS + tid] += red[RD_MV_THREADS + tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (with_obs) {
        slot[0] = red[0];
        slot[1] = red[RD_MV_THREADS];
      } else {
        slot[0] = red[RD_MV_THREADS];
      }
    }
  }
}

// One workgroup per day.  Per-day form: slots [D][NT][2].  Shared form: member slots [1 + D][NT] (block 0 when the day has no
// NaN, else block 1 + d), observation slots [T][ldo] with the day as the column.
__global__ void __launch_bounds__(RD_MV_THREADS)
k_mv_energy_reduce(const double* __restrict__ slots, const double* __restrict__ obs_slots, long NT, int T, long ldo, int shared, long P,
                   const long long* __restrict__ nvalid, double* __restrict__ obs_sum, double* __restrict__ pair_sum) {
  __shared__ double red[2][RD_MV_THREADS];
  const long day = blockIdx.x;
  const int tid = threadIdx.x;
  const long long nv = nvalid[day];
  double so = 0.0, sp = 0.0;
  if (nv > 0) {                                                            // (the same in the whole workgroup)
    if (shared) {
      const double* ps = slots + (nv == P ? 0 : 1 + day) * NT;
      for (long s = tid; s < NT; s += RD_MV_THREADS) sp += ps[s];
      for (long s = tid; s < T; s += RD_MV_THREADS) so += obs_slots[s * ldo + day];
    } else {
      const double* ps = slots + day * NT * 2;
      for (long s = tid; s < NT; s += RD_MV_THREADS) {
        so += ps[2 * s];
        sp += ps[2 * s + 1];
      }
    }
  }
  red[0][tid] = so;
  red[1][tid] = sp;
  __syncthreads();
  for (int s = RD_MV_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    obs_sum[day] = nv > 0 ? red[0][0] : nan;
    pair_sum[day] = nv > 0 ? red[1][0] : nan;
  }
}

// ---- variogram score
struct rd_mv_slot {
  double sq;
  long long count;
};

// MODE 0: members and score, grid = days x units; MODE 1: members only, means to `table`, grid = units; MODE 2: score from `table`,
// grid = days x units.  ens: the day's members [m][24 plane] at ens + day * ens_day_stride.
template <int MODE, bool HALF>
__global__ void __launch_bounds__(RD_MV_THREADS)
k_mv_variogram(const float* __restrict__ ens, long ens_day_stride, const float* __restrict__ obs, int m, int ny, int nx, int R, int L,
               double* __restrict__ table, rd_mv_slot* __restrict__ slots) {
  constexpr int BMAX = (RD_MV_VT + 2 * RD_MV_MAXR) * (RD_MV_VT + 2 * RD_MV_MAXR);           // 576
  __shared__ float btile[2][BMAX];
  __shared__ float ytile[BMAX];
  __shared__ int dofs[RD_MV_VG];
  __shared__ double wsq[RD_MV_THREADS / 64][RD_MV_VG];
  __shared__ int wcnt[RD_MV_THREADS / 64][RD_MV_VG];
  const int tid = threadIdx.x, tx = tid & (RD_MV_VT - 1), ty = tid / RD_MV_VT;
  const long plane = (long)ny * nx, P = RD_HOURS * plane;
  const int ntx = (nx + RD_MV_VT - 1) / RD_MV_VT;
  const long nt = rd_mv_vtiles(ny, nx), U = rd_mv_units(ny, nx, R, L);
  const long day = blockIdx.x / U;
  long u = blockIdx.x % U;
  int l = 0;
  for (;;) {                                                               // the unit -> lag, hour, group, tile
    const long n = (long)(RD_HOURS - l) * rd_mv_groups(R, l) * nt;
    if (u < n) break;
    u -= n;
    ++l;
  }
  const int ng = rd_mv_groups(R, l);
  const int h = (int)(u / (ng * nt)), g = (int)(u / nt % ng), tile = (int)(u % nt);
  const int y0 = tile / ntx * RD_MV_VT, x0 = tile % ntx * RD_MV_VT;
  const int side = rd_mv_side(R), bside = RD_MV_VT + 2 * R, belems = bside * bside;
  const int d0 = rd_mv_first(R, l) + g * RD_MV_VG;                         // the group's first displacement
  const int nd = side * side - d0 < RD_MV_VG ? side * side - d0 : RD_MV_VG;
  if (tid < RD_MV_VG) {
    const int d = d0 + (tid < nd ? tid : 0);
    dofs[tid] = (d / side - R) * bside + (d % side - R);        // offset in the B tile from the anchor's own place
  }

  // what this thread stages of the B tile (hour h + l, rows y0 - R .., columns x0 - R ..): up to 3 elements
  long boff[3];
  bool bin[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int e = tid + RD_MV_THREADS * q;
    const int y = y0 - R + e / bside, x = x0 - R + e % bside;
    bin[q] = e < belems && y >= 0 && y < ny && x >= 0 && x < nx;
    boff[q] = bin[q] ? (long)(h + l) * plane + (long)y * nx + x : 0;
  }
  const bool ain = y0 + ty < ny && x0 + tx < nx;
  const long aoff = ain ? (long)h * plane + (long)(y0 + ty) * nx + x0 + tx : 0;
  const int acentre = (ty + R) * bside + tx + R;

  double acc[RD_MV_VG];
#pragma unroll
  for (int k = 0; k < RD_MV_VG; ++k) acc[k] = 0.0;

  if constexpr (MODE != 2) {
    const float* e = ens + day * ens_day_stride;
    float a_next = ain ? e[aoff] : 0.0f, b_next[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) b_next[q] = bin[q] ? e[boff[q]] : 0.0f;
    for (int k = 0; k < m; ++k) {
      const int buf = k & 1;
      const float a = a_next;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (tid + RD_MV_THREADS * q < belems) btile[buf][tid + RD_MV_THREADS * q] = b_next[q];
      __syncthreads();                                                     // (also publishes dofs; buffer buf was last read before the barrier of member k - 1)
      if (k + 1 < m) {
        const float* en = e + (long)(k + 1) * P;
        a_next = ain ? en[aoff] : 0.0f;
#pragma unroll
        for (int q = 0; q < 3; ++q) b_next[q] = bin[q] ? en[boff[q]] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < RD_MV_VG; ++i)
        if (i < nd) {                                                      // (the same in the whole workgroup)
          float v = fabsf(__fsub_rn(a, btile[buf][acentre + dofs[i]]));
          if constexpr (HALF) v = sqrtf(v);
          acc[i] += (double)v;
        }
    }
#pragma unroll
    for (int i = 0; i < RD_MV_VG; ++i) acc[i] = acc[i] / (double)m;
  }
  if constexpr (MODE == 1) {
    double* t = table + (long)blockIdx.x * RD_MV_VG * RD_MV_THREADS;
#pragma unroll
    for (int i = 0; i < RD_MV_VG; ++i) t[i * RD_MV_THREADS + tid] = acc[i];
    return;
  } else {
    if constexpr (MODE == 2) {
      const double* t = table + (blockIdx.x % U) * RD_MV_VG * RD_MV_THREADS;
#pragma unroll
      for (int i = 0; i < RD_MV_VG; ++i) acc[i] = t[i * RD_MV_THREADS + tid];
    }
    const float* y = obs + day * P;
    const float nanf_ = __uint_as_float(0x7FC00000u);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (tid + RD_MV_THREADS * q < belems) ytile[tid + RD_MV_THREADS * q] = bin[q] ? y[boff[q]] : nanf_;
    const float ya = ain ? y[aoff] : nanf_;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < RD_MV_VG; ++i) {
      double term = 0.0;
      int cnt = 0;
      if (i < nd) {
        const float yb = ytile[acentre + dofs[i]];
        if (!rd_mv_nan(ya) && !rd_mv_nan(yb)) {
          float o = fabsf(__fsub_rn(ya, yb));
          if constexpr (HALF) o = sqrtf(o);
          const double df = __dsub_rn((double)o, acc[i]);
          term = __dmul_rn(df, df);
          cnt = 1;
        }
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {                                   // a fixed tree over the wave
        term = __dadd_rn(term, __shfl_xor(term, s));
        cnt += __shfl_xor(cnt, s);
      }
      if (lane == 0) {
        wsq[wave][i] = term;
        wcnt[wave][i] = cnt;
      }
    }
    __syncthreads();
    if (tid < RD_MV_VG) {
      rd_mv_slot s;
      s.sq = __dadd_rn(__dadd_rn(wsq[0][tid], wsq[1][tid]), __dadd_rn(wsq[2][tid], wsq[3][tid]));
      s.count = (long long)wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
      slots[(long)blockIdx.x * RD_MV_VG + tid] = s;
    }
  }
}

// one thread per (day, lag, displacement of the full (2R + 1)^2 table): the slots of its hours and tiles in order; 0 outside the
// half-space, NaN / 0 for a day without a valid position
__global__ void __launch_bounds__(RD_MV_THREADS)
k_mv_variogram_reduce(const rd_mv_slot* __restrict__ slots, long n_days, int ny, int nx, int R, int L, const long long* __restrict__ nvalid,
                      double* __restrict__ sq_out, long long* __restrict__ count_out) {
  const int S2 = rd_mv_side(R) * rd_mv_side(R);
  const long idx = (long)blockIdx.x * RD_MV_THREADS + threadIdx.x;
  if (idx >= n_days * (L + 1) * S2) return;
  const int d = (int)(idx % S2), l = (int)(idx / S2 % (L + 1));
  const long day = idx / ((long)S2 * (L + 1));
  double sq = 0.0;
  long long cnt = 0;
  const int first = rd_mv_first(R, l);
  if (d >= first) {
    const long nt = rd_mv_vtiles(ny, nx), U = rd_mv_units(ny, nx, R, L);
    const int ng = rd_mv_groups(R, l), g = (d - first) / RD_MV_VG, k = (d - first) % RD_MV_VG;
    const rd_mv_slot* base = slots + (day * U + rd_mv_unit_base(ny, nx, R, l)) * RD_MV_VG + k;
    for (int h = 0; h < RD_HOURS - l; ++h)
      for (long t = 0; t < nt; ++t) {
        const rd_mv_slot s = base[(((long)h * ng + g) * nt + t) * RD_MV_VG];
        sq = __dadd_rn(sq, s.sq);
        cnt += s.count;
      }
    if (nvalid[day] == 0) sq = __longlong_as_double(0x7FF8000000000000LL);
  }
  sq_out[idx] = sq;
  count_out[idx] = cnt;
}
