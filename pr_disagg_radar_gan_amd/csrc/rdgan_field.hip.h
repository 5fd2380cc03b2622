// Whole daily fields through the generator: the field is cut into overlapping nd x nd tiles, every tile that
// holds rain is disaggregated by the generator, and the tiles' hourly fractions are blended back into the field.
//
// Tile plan (the host states it, the kernels only evaluate it): step = nd - overlap; tile i of an axis of length L starts at
// rd_field_origin(i) = min(i * step, L - nd); there are rd_field_axis_tiles(L) = ceil((L - nd) / step) + 1 of them (the regular ones
// at 0, step, 2 step, ... plus one flush with the end when those stop short of it).  Tiles are numbered y-major, tile = iy * n_tx + ix.
//
//  * k_field_scan:  per (day, tile) the number of wet (finite, > 0), NaN and bad (negative or infinite) pixels.  Integer counts, so
//    the order of the sweep does not matter.
//  * k_field_cond:  the generator's condition batch for a list of (day, tile) entries: daily / norm_scale (fp64 quotient rounded to
//    fp32, as raindisagg_gan_pretrained.generate_scenarios forms it), a NaN pixel entering as 0.
//  * k_field_blend: out[u, h, y, x] = daily[day(u), y, x] * sum over the tiles covering (y, x) of wy * wx * frac[slot(u, tile), h, y - oy, x - ox]
//    for a group of whole (scenario, day) units u.  Each element of frac is read by exactly one thread and each element of out is
//    written by exactly one thread: no atomics, and the sum of a pixel runs in a fixed order (y entries outer, x entries inner), so
//    two calls agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_FIELD_THREADS 256
#define RD_FIELD_BX 64          // a wave takes 64 adjacent x of one field row,
#define RD_FIELD_BY 4           // the four waves of a workgroup four adjacent rows: they share the tile rows they read
#define RD_FIELD_COVER 3        // at most 3 tiles cover a coordinate per axis (overlap <= nd / 2)

__host__ __device__ __forceinline__ int rd_field_origin(int i, int step, int L, int nd) {
  const long o = (long)i * step;
  return o < (long)(L - nd) ? (int)o : L - nd;
}
static inline int rd_field_axis_tiles(int L, int nd, int step) { return (L - nd + step - 1) / step + 1; }

// One wave per (day, tile), four per workgroup; counts[(day * T + tile) * 3 + {0, 1, 2}] = wet, NaN, bad.
__global__ void __launch_bounds__(RD_FIELD_THREADS)
k_field_scan(const float* __restrict__ daily, long n_entries, int ny, int nx, int nd, int step, int n_ty, int n_tx,
             int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long plane = (long)ny * nx;
  const int T = n_ty * n_tx;
  for (long e = blockIdx.x * 4L + (threadIdx.x >> 6); e < n_entries; e += gridDim.x * 4L) {
    const long day = e / T;
    const int t = (int)(e - day * T);
    const int oy = rd_field_origin(t / n_tx, step, ny, nd), ox = rd_field_origin(t % n_tx, step, nx, nd);
    const float* p = daily + day * plane + (long)oy * nx + ox;
    int wet = 0, nan = 0, bad = 0;
    for (int pix = lane; pix < nd * nd; pix += 64) {
      const float v = p[(long)(pix / nd) * nx + pix % nd];
      const bool inf = fabsf(v) == __builtin_inff();
      nan += v != v;
      bad += (v < 0.f) || inf;
      wet += (v > 0.f) && !inf;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      wet += __shfl_down(wet, off, 64);
      nan += __shfl_down(nan, off, 64);
      bad += __shfl_down(bad, off, 64);
    }
    if (lane == 0) {
      counts[3 * e] = wet;
      counts[3 * e + 1] = nan;
      counts[3 * e + 2] = bad;
    }
  }
}

// One thread per (entry, i, j) of the batch, adjacent threads adjacent j; entries[e] = day * T + tile (checked by the host).
__global__ void __launch_bounds__(RD_FIELD_THREADS)
k_field_cond(const float* __restrict__ daily, const int* __restrict__ entries, long m, int ny, int nx, int nd, int step, int n_ty,
             int n_tx, double norm_scale, float* __restrict__ cond) {
  const long plane = (long)ny * nx, total = m * nd * nd;
  const int T = n_ty * n_tx;
  for (long f = blockIdx.x * (long)RD_FIELD_THREADS + threadIdx.x; f < total; f += (long)gridDim.x * RD_FIELD_THREADS) {
    const int j = (int)(f % nd), i = (int)((f / nd) % nd);
    const int e = entries[f / ((long)nd * nd)];
    const long day = e / T;
    const int t = e % T;
    const int oy = rd_field_origin(t / n_tx, step, ny, nd), ox = rd_field_origin(t % n_tx, step, nx, nd);
    const float v = daily[day * plane + (long)(oy + i) * nx + (ox + j)];
    cond[f] = v != v ? 0.f : (float)((double)v / norm_scale);
  }
}

// The per-pixel resolve k_field_blend and k_field_blend_peaks (rdgan_products.hip.h) share: the (at most 9) covering tiles of
// pixel (y, x) of a unit whose slot row is srow, as off[k] = the offset of the pixel's hour 0 in frac (-1: the tile contributes
// nothing) and w[k] = wy * wx, y entries outer and x entries inner.  A table entry that does not cover its coordinate is ignored.
__device__ __forceinline__ void rd_field_resolve(const int* __restrict__ srow, const int* __restrict__ ytab_i,
                                                 const float* __restrict__ ytab_w, const int* __restrict__ xtab_i,
                                                 const float* __restrict__ xtab_w, int y, int x, int ny, int nx, int nd, int step,
                                                 int n_ty, int n_tx, long (&off)[RD_FIELD_COVER * RD_FIELD_COVER],
                                                 float (&w)[RD_FIELD_COVER * RD_FIELD_COVER]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < RD_FIELD_COVER; ++a) {
    const int iy = ytab_i[y * RD_FIELD_COVER + a];
    const float wy = ytab_w[y * RD_FIELD_COVER + a];
    const bool oky = iy >= 0 && iy < n_ty;
    const int ty = y - rd_field_origin(oky ? iy : 0, step, ny, nd);
#pragma unroll
    for (int c = 0; c < RD_FIELD_COVER; ++c) {
      const int ix = xtab_i[x * RD_FIELD_COVER + c];
      const float wx = xtab_w[x * RD_FIELD_COVER + c];
      const bool okx = ix >= 0 && ix < n_tx;
      const int tx = x - rd_field_origin(okx ? ix : 0, step, nx, nd);
      const bool ok = oky && okx && ty >= 0 && ty < nd && tx >= 0 && tx < nd;
      const int slot = ok ? srow[iy * n_tx + ix] : -1;
      off[a * RD_FIELD_COVER + c] = slot >= 0 ? ((long)slot * RD_HOURS * nd + ty) * nd + tx : -1;
      w[a * RD_FIELD_COVER + c] = wy * wx;
    }
  }
}

// hour h of a resolved pixel: d * sum_k w[k] * frac[off[k] + h * tile], the products rounded before they are added, k ascending
__device__ __forceinline__ float rd_field_hour(const float* __restrict__ frac, const long (&off)[RD_FIELD_COVER * RD_FIELD_COVER],
                                               const float (&w)[RD_FIELD_COVER * RD_FIELD_COVER], int h, long tile, float d) {
#pragma clang fp contract(off)
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < RD_FIELD_COVER * RD_FIELD_COVER; ++k)
    if (off[k] >= 0) acc = acc + w[k] * frac[off[k] + h * tile];
  return d * acc;
}

// A workgroup takes a 4 x 64 patch of one unit's field and walks the 24 hours; lane = x, so a wave reads nd contiguous floats per
// tile row it crosses and writes 64 contiguous floats of an output row.  The (at most 9) covering tiles of a pixel are resolved once,
// into registers; per hour a pixel then costs its loads, as many multiply-adds, one multiply and one store.
//   frac  [m][24][nd][nd]        the generator's output as rdgan_gen_forward leaves it
//   slots [units][T]             row of frac holding (unit, tile), -1: the tile was skipped (it contributes nothing)
//   ytab_i / ytab_w [ny][3], xtab_i / xtab_w [nx][3]: the tiles along the axis covering the coordinate (-1: none) and their weights
//   daily [n_days][ny][nx]; unit u of the group is day (first_unit + u) % n_days;  out [units][24][ny][nx]
// A dry pixel (daily == 0) gives 0 and a NaN pixel NaN whatever the fractions hold; neither reads frac.  An entry of a table that
// does not cover its coordinate is ignored, so a wrong table cannot make the kernel read outside frac.  All offsets are 64-bit.
__global__ void __launch_bounds__(RD_FIELD_THREADS)
k_field_blend(const float* __restrict__ frac, const int* __restrict__ slots, const int* __restrict__ ytab_i,
              const float* __restrict__ ytab_w, const int* __restrict__ xtab_i, const float* __restrict__ xtab_w,
              const float* __restrict__ daily, float* __restrict__ out, long units, long first_unit, long n_days, int ny, int nx,
              int nd, int step, int n_ty, int n_tx) {
#pragma clang fp contract(off)
  const int lx = threadIdx.x & (RD_FIELD_BX - 1), ly = threadIdx.x / RD_FIELD_BX;
  const long plane = (long)ny * nx, tile = (long)nd * nd;
  const int T = n_ty * n_tx;
  const long nbx = (nx + RD_FIELD_BX - 1) / RD_FIELD_BX, nby = (ny + RD_FIELD_BY - 1) / RD_FIELD_BY;
  const long n_blocks = units * nby * nbx;
  for (long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const long u = b / (nby * nbx);
    const int y = (int)((b / nbx) % nby) * RD_FIELD_BY + ly, x = (int)(b % nbx) * RD_FIELD_BX + lx;
    if (y >= ny || x >= nx) continue;
    const float d = daily[((first_unit + u) % n_days) * plane + (long)y * nx + x];
    float* dst = out + u * RD_HOURS * plane + (long)y * nx + x;
    if (d == 0.f || d != d) {
#pragma unroll
      for (int h = 0; h < RD_HOURS; ++h) dst[h * plane] = d;         // 0 stays 0, NaN stays NaN
      continue;
    }
    long off[RD_FIELD_COVER * RD_FIELD_COVER];
    float w[RD_FIELD_COVER * RD_FIELD_COVER];
    rd_field_resolve(slots + u * T, ytab_i, ytab_w, xtab_i, xtab_w, y, x, ny, nx, nd, step, n_ty, n_tx, off, w);
#pragma unroll 4
    for (int h = 0; h < RD_HOURS; ++h) dst[h * plane] = rd_field_hour(frac, off, w, h, tile, d);
  }
}
