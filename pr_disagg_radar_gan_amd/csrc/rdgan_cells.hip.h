// Rain cells of hourly fields: connected wet areas of every (day, hour) plane, labelled and counted.
// x [n][24][ny][nx] fp32 with a leading stride day_stride >= 24 ny nx.  A plane is one (i, h); a pixel is wet for threshold t when
// x > thr[t] in fp32 and it is finite, bad when it is NaN or +-inf (never wet).  A cell is a maximal set of wet pixels of one plane
// connected under 4- or 8-connectivity; its canonical label is its smallest flat index y nx + x.
//
// The workspace holds, for the P planes of a pass, three maps over [P][ny nx]: parent (int32: a union-find forest over plane
// indices, -1 for a pixel that is not wet), area (uint32, bit 31 the edge flag) and vol (uint64), and two words per plane.
//
//  * k_cells_label_tile: one workgroup per (plane, tile of at most 64 x 64).  A wave's ballot of the compare is the wet mask of
//    a tile row.  Every wet pixel starts with the first pixel of its row run as parent (from the masks, no union needed along a
//    row) and is united with the row above where the masks say the two runs first touch; the union-find lives in LDS.  Area,
//    volume and edge flag are summed per local root in LDS, and every pixel of the tile writes its maps: parent = the plane index
//    of its local root, area = the local sums if it IS a local root and 0 otherwise (so the maps need no clearing).
//  * k_cells_merge: one thread per pixel pair across a tile border (and the diagonal pairs for 8-connectivity, corners included)
//    unites the two in the workspace map with atomicMin; every read of parent there is a relaxed agent-scope atomic load.
//  * k_cells_resolve: one thread per pixel finds its final root, writes it back (and the label map when asked), and a local root
//    that is not a final root adds its sums to the final root's slots: one integer atomic per (tile, local cell) and quantity.
//  * k_cells_reduce: every final root bins its cell into a per-workgroup LDS table, which is merged into the state with 64-bit
//    integer atomics; the count and the largest area of a plane are formed with one atomic add and one atomic max per wave.
//  * k_cells_planes: one thread per plane bins the plane's count and largest area.
//
// THE INVARIANT, in LDS and in the workspace alike: parent[i] <= i whenever parent[i] >= 0, and parent[] only ever decreases
// (atomicMin).  A find therefore descends strictly until it meets a root and ends after at most i steps; a union loop strictly
// lowers the larger of its two indices and ends too, whatever order the hardware picks.  Kernel boundaries are the only ordering
// between the phases: no spin-wait, no grid sync.  No floating-point atomics.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_CL_MAXT RD_THR_MAX
#define RD_CL_TILE 64
#define RD_CL_THREADS 256
#define RD_CL_MAXPASS 65535              // planes of one pass: the grid's y
#define RD_CL_NBINS 25                   // floor(log2(area)) = 0 .. 24
#define RD_CL_NKP 65                     // cells_per_plane[0 .. 64], the last bin open
#define RD_CL_RCHUNK 4096                // pixels of a plane one workgroup of k_cells_reduce takes
// the state: counters per threshold, flat
#define RD_CL_WET 0                      // wet_pixels[24]
#define RD_CL_CELLS 24                   // cells[2][24]
#define RD_CL_HIST 72                    // area_hist[2][25]
#define RD_CL_ASUM 122                   // area_sum[2]
#define RD_CL_ASQ 124                    // area_sq_sum[2]
#define RD_CL_VBA 126                    // volume_by_area[2][25]
#define RD_CL_KPP 176                    // cells_per_plane[65]
#define RD_CL_LARGEST 241                // largest_area[25]
#define RD_CL_DRY 266                    // dry_planes
#define RD_CL_ABA 267                    // area_by_area[2][25]
#define RD_CL_NC 317
// the LDS table of k_cells_reduce (one plane, so one hour): cells[2], hist[2][25], asum[2], asq[2], vba[2][25], aba[2][25]
#define RD_CL_LCELLS 0
#define RD_CL_LHIST 2
#define RD_CL_LASUM 52
#define RD_CL_LASQ 54
#define RD_CL_LVBA 56
#define RD_CL_LABA 106
#define RD_CL_NL 156
#define RD_CL_EDGE 0x80000000u

// bytes of the workspace for P planes of `plane` pixels: vol, parent, area, then count and max per plane
__host__ __device__ inline long rd_cl_ws_bytes(long plane, long P) { return P * plane * 16 + P * 8; }
// dynamic LDS of k_cells_label_tile: vol[4096] u64, parent[4096] int, area[4096] u32, wet[64] and bad[66] row masks, two halo
// columns of 66 flags packed in 4 words each side, 2 counters
#define RD_CL_LDS_BYTES (4096 * 16 + (64 + 66 + 4) * 8 + 16)

__device__ __forceinline__ int rd_cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int rd_cl_load_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// -> the root of i.  Bound: parent[j] <= j, so every step that does not end the loop lowers i: at most i steps.
template <bool LDS> __device__ __forceinline__ int rd_cl_find(const int* parent, int i) {
  for (;;) {
    const int q = LDS ? rd_cl_load_lds(parent + i) : rd_cl_load(parent + i);
    if (q == i) return i;
    i = q;
  }
}

// unite the sets of a and b: the larger index is hooked under the smaller with atomicMin.  Bound: an iteration that does not end
// the loop replaces the larger index a by the value old < a that parent[a] held, so max(a, b) strictly decreases: at most
// max(a, b) iterations.  parent[a] <= a is kept because b < a is all atomicMin can write.
template <bool LDS> __device__ __forceinline__ void rd_cl_union(int* parent, int a, int b) {
  a = rd_cl_find<LDS>(parent, a);
  b = rd_cl_find<LDS>(parent, b);
  while (a != b) {
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;                                                  // a was a root and now hangs under b
    a = old;                                                              // a hung under old already: unite old and b
  }
}

// q(x) = rint(min(x, 2^20) 2^16): exact in fp64, rounded half to even once
__device__ __forceinline__ unsigned long long rd_cl_q(float x) {
  const double d = fmin((double)x, 1048576.0) * 65536.0;
  return (unsigned long long)(long long)__builtin_rint(d);
}

__global__ void __launch_bounds__(RD_CL_THREADS)
k_cells_label_tile(const float* __restrict__ x, long day_stride, int ny, int nx, long plane0, float thr, int conn8, int count_bad,
                   unsigned long long* __restrict__ wet_counts, unsigned long long* __restrict__ bad_count,
                   unsigned long long* __restrict__ vol_ws, int* __restrict__ parent_ws, unsigned* __restrict__ area_ws,
                   unsigned* __restrict__ plane_words) {
  extern __shared__ unsigned long long rd_cl_lds[];
  unsigned long long* lvol = rd_cl_lds;                                    // [4096]
  int* lpar = reinterpret_cast<int*>(rd_cl_lds + 4096);                    // [4096]
  unsigned* larea = reinterpret_cast<unsigned*>(lpar + 4096);              // [4096]
  unsigned long long* wetm = rd_cl_lds + 4096 * 2;                         // [64]
  unsigned long long* badm = wetm + 64;                                    // [66]: tile rows -1 .. 64
  unsigned* halo = reinterpret_cast<unsigned*>(badm + 66);                 // [2][4]: bit r + 1 of side s: the pixel beside row r is bad
  unsigned* cnt = halo + 8;                                                // wet, bad

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (nx + RD_CL_TILE - 1) / RD_CL_TILE;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const int y0 = ty * RD_CL_TILE, x0 = tx * RD_CL_TILE;
  const long pl = blockIdx.y, gp = plane0 + pl, plane = (long)ny * nx;
  const float* src = x + (gp / RD_HOURS) * day_stride + (gp % RD_HOURS) * plane;
  const long wbase = pl * plane;

  if (tid < 10) halo[tid] = 0u;                                            // (halo[8], halo[9] are cnt)
  for (int i = tid; i < 4096; i += RD_CL_THREADS) {
    lvol[i] = 0ull;
    larea[i] = 0u;
  }
  if (blockIdx.x == 0 && tid < 2) plane_words[pl * 2 + tid] = 0u;          // the plane's cell count and largest area
  __syncthreads();

  // the masks.  Row r of the tile is owned by wave r % 4, column c by lane c; a pixel outside the plane is dry and not bad.
  unsigned long long q[16];
  unsigned n_wet = 0, n_bad = 0;
  const int gx = x0 + lane;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i, gy = y0 + r;
    float v = 0.0f;
    if (gy < ny && gx < nx) v = src[(long)gy * nx + gx];
    const bool bad = ((__float_as_uint(v) & RD_F32_EXP) == RD_F32_EXP);
    const bool wet = !bad && v > thr;
    const unsigned long long wm = __ballot(wet), bm = __ballot(bad);
    q[i] = wet ? rd_cl_q(v) : 0ull;
    n_wet += (unsigned)__popcll(wm);
    n_bad += (unsigned)__popcll(bm);
    if (lane == 0) {
      wetm[r] = wm;
      badm[r + 1] = bm;
    }
  }
  if (wave < 2) {                                                          // the rows above and below the tile
    const int gy = wave == 0 ? y0 - 1 : y0 + RD_CL_TILE;
    float v = 0.0f;
    if (gy >= 0 && gy < ny && gx < nx) v = src[(long)gy * nx + gx];
    const unsigned long long bm = __ballot(((__float_as_uint(v) & RD_F32_EXP) == RD_F32_EXP));
    if (lane == 0) badm[wave == 0 ? 0 : 65] = bm;
  }
  if (tid < 132) {                                                         // the columns left and right of the tile, rows -1 .. 64
    const int side = tid / 66, rr = tid % 66, gy = y0 + rr - 1, hx = side == 0 ? x0 - 1 : x0 + RD_CL_TILE;
    if (gy >= 0 && gy < ny && hx >= 0 && hx < nx) {
      const float v = src[(long)gy * nx + hx];
      if (((__float_as_uint(v) & RD_F32_EXP) == RD_F32_EXP)) atomicOr(&halo[side * 4 + (rr >> 5)], 1u << (rr & 31));
    }
  }
  if (lane == 0) {
    if (n_wet) atomicAdd(&cnt[0], n_wet);
    if (n_bad) atomicAdd(&cnt[1], n_bad);
  }
  __syncthreads();

  // every wet pixel starts under the first pixel of its row run
  bool wet[16], edge[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i, gy = y0 + r;
    const unsigned long long m = wetm[r];
    wet[i] = (m >> lane) & 1ull;
    const unsigned long long below = ~m & ((1ull << lane) - 1ull);         // the dry pixels left of this one
    const int start = below ? 64 - __builtin_clzll(below) : 0;
    lpar[r * 64 + lane] = wet[i] ? r * 64 + start : -1;
    // bad in the 8-neighbourhood, or on the rim of the plane
    unsigned long long nb = 0ull;
#pragma unroll
    for (int rr = r; rr <= r + 2; ++rr) {                                  // badm / halo index of tile rows r - 1 .. r + 1
      const unsigned long long b = badm[rr];
      nb |= b | (b << 1) | (b >> 1);
      nb |= (unsigned long long)((halo[rr >> 5] >> (rr & 31)) & 1u);
      nb |= (unsigned long long)((halo[4 + (rr >> 5)] >> (rr & 31)) & 1u) << 63;
    }
    edge[i] = ((nb >> lane) & 1ull) || gy == 0 || gy == ny - 1 || gx == 0 || gx == nx - 1;
  }
  __syncthreads();

  // unite with the row above.  Where the pixel to the left and the one above it are both wet, that pair has united the two runs
  // already (or the pair left of it has, by induction along the overlap).
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i;
    if (r == 0 || !wet[i]) continue;
    const unsigned long long up = wetm[r - 1], cur = wetm[r];
    const int p = r * 64 + lane, u = p - 64;
    const bool left_pair = lane > 0 && ((cur >> (lane - 1)) & (up >> (lane - 1)) & 1ull);
    if ((up >> lane) & 1ull) {
      if (!left_pair) rd_cl_union<true>(lpar, p, u);
    } else if (conn8) {
      if (lane > 0 && ((up >> (lane - 1)) & 1ull)) rd_cl_union<true>(lpar, p, u - 1);
      if (lane < 63 && ((up >> (lane + 1)) & 1ull)) rd_cl_union<true>(lpar, p, u + 1);
    }
  }
  __syncthreads();

  // the sums of every local root (no union runs any more: the roots are fixed)
  int root[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    root[i] = -1;
    if (!wet[i]) continue;
    root[i] = rd_cl_find<true>(lpar, (wave + 4 * i) * 64 + lane);
    atomicAdd(&larea[root[i]], 1u);
    if (edge[i]) atomicOr(&larea[root[i]], RD_CL_EDGE);
    atomicAdd(&lvol[root[i]], q[i]);
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i, gy = y0 + r;
    if (gy >= ny || gx >= nx) continue;
    const long g = wbase + (long)gy * nx + gx;
    const int p = r * 64 + lane;
    // (row-major inside the tile and inside the plane agree on the order: the local root is the smallest plane index too)
    parent_ws[g] = wet[i] ? (y0 + (root[i] >> 6)) * nx + x0 + (root[i] & 63) : -1;
    const bool is_root = wet[i] && root[i] == p;
    area_ws[g] = is_root ? larea[p] : 0u;
    if (is_root) vol_ws[g] = lvol[p];
  }
  if (tid == 0) {
    if (cnt[0]) atomicAdd(&wet_counts[gp % RD_HOURS], (unsigned long long)cnt[0]);
    if (count_bad && cnt[1]) atomicAdd(bad_count, (unsigned long long)cnt[1]);
  }
}

// item < (tiles_x - 1) ny: the pixel left of a vertical border and its 1 or 3 neighbours right of it; the others: the pixel
// above a horizontal border and its 1 or 3 neighbours below it (the diagonal across a corner of four tiles is among both)
__global__ void __launch_bounds__(RD_CL_THREADS)
k_cells_merge(int ny, int nx, int conn8, int* __restrict__ parent_ws) {
  const int tiles_x = (nx + RD_CL_TILE - 1) / RD_CL_TILE, tiles_y = (ny + RD_CL_TILE - 1) / RD_CL_TILE;
  const long nvert = (long)(tiles_x - 1) * ny, items = nvert + (long)(tiles_y - 1) * nx;
  const long it = (long)blockIdx.x * RD_CL_THREADS + threadIdx.x;
  if (it >= items) return;
  int* parent = parent_ws + (long)blockIdx.y * ny * nx;
  int ay, ax, dy, dx;                                                      // a, and the direction across the border
  if (it < nvert) {
    ay = (int)(it % ny);
    ax = (int)(it / ny + 1) * RD_CL_TILE - 1;
    dy = 0;
    dx = 1;
  } else {
    const long j = it - nvert;
    ay = (int)(j / nx + 1) * RD_CL_TILE - 1;
    ax = (int)(j % nx);
    dy = 1;
    dx = 0;
  }
  const int a = ay * nx + ax;
  if (rd_cl_load(parent + a) < 0) return;
  for (int s = conn8 ? -1 : 0; s <= (conn8 ? 1 : 0); ++s) {
    const int by = ay + dy + (dx ? s : 0), bx = ax + dx + (dy ? s : 0);
    if (by < 0 || by >= ny || bx < 0 || bx >= nx) continue;
    const int b = by * nx + bx;
    if (rd_cl_load(parent + b) >= 0) rd_cl_union<false>(parent, a, b);
  }
}

__global__ void __launch_bounds__(RD_CL_THREADS)
k_cells_resolve(long plane, long plane0, unsigned long long* __restrict__ vol_ws, int* __restrict__ parent_ws,
                unsigned* __restrict__ area_ws, int* __restrict__ labels) {
  const long p = (long)blockIdx.x * RD_CL_THREADS + threadIdx.x;
  if (p >= plane) return;
  const long base = (long)blockIdx.y * plane;
  int* parent = parent_ws + base;
  int r = rd_cl_load(parent + p);
  if (r >= 0) {
    r = rd_cl_find<false>(parent, r);
    // a local root under another root hands its sums on.  Nobody adds to ITS slots (only final roots receive), and a final
    // root's slots are read by nobody in this kernel.
    const unsigned a = area_ws[base + p];
    if (a && r != (int)p) {
      atomicAdd(&area_ws[base + r], a & ~RD_CL_EDGE);
      if (a & RD_CL_EDGE) atomicOr(&area_ws[base + r], RD_CL_EDGE);
      atomicAdd(&vol_ws[base + r], vol_ws[base + p]);
    }
    // (another thread's find may pass through p meanwhile: it reads the old parent or the root, both above it in its tree)
    __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (labels) labels[(plane0 + blockIdx.y) * plane + p] = r;
}

__global__ void __launch_bounds__(RD_CL_THREADS)
k_cells_reduce(long plane, long plane0, const unsigned long long* __restrict__ vol_ws, const int* __restrict__ parent_ws,
               const unsigned* __restrict__ area_ws, unsigned* __restrict__ plane_words, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long tab[RD_CL_NL];
  const int tid = threadIdx.x;
  for (int i = tid; i < RD_CL_NL; i += RD_CL_THREADS) tab[i] = 0ull;
  __syncthreads();
  const long base = (long)blockIdx.y * plane, p0 = (long)blockIdx.x * RD_CL_RCHUNK;
  unsigned n = 0, amax = 0;
#pragma unroll 4
  for (int k = 0; k < RD_CL_RCHUNK / RD_CL_THREADS; ++k) {
    const long p = p0 + k * RD_CL_THREADS + tid;
    if (p >= plane || parent_ws[base + p] != (int)p) continue;
    const unsigned w = area_ws[base + p], a = w & ~RD_CL_EDGE, c = w >> 31;
    const int b = 31 - __builtin_clz(a);                                   // (a root has a >= 1)
    ++n;
    amax = a > amax ? a : amax;
    atomicAdd(&tab[RD_CL_LCELLS + c], 1ull);
    atomicAdd(&tab[RD_CL_LHIST + c * RD_CL_NBINS + b], 1ull);
    atomicAdd(&tab[RD_CL_LASUM + c], (unsigned long long)a);
    atomicAdd(&tab[RD_CL_LASQ + c], (unsigned long long)a * a);
    atomicAdd(&tab[RD_CL_LVBA + c * RD_CL_NBINS + b], vol_ws[base + p]);
    atomicAdd(&tab[RD_CL_LABA + c * RD_CL_NBINS + b], (unsigned long long)a);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    n += __shfl_xor(n, s);
    const unsigned o = __shfl_xor(amax, s);
    amax = o > amax ? o : amax;
  }
  if ((tid & 63) == 0 && n) {
    atomicAdd(&plane_words[blockIdx.y * 2], n);
    atomicMax(&plane_words[blockIdx.y * 2 + 1], amax);
  }
  __syncthreads();
  const int h = (int)((plane0 + blockIdx.y) % RD_HOURS);
  for (int i = tid; i < RD_CL_NL; i += RD_CL_THREADS) {
    const unsigned long long v = tab[i];
    if (!v) continue;
    int dst;
    if (i < RD_CL_LHIST) dst = RD_CL_CELLS + i * RD_HOURS + h;
    else if (i < RD_CL_LASUM) dst = RD_CL_HIST + (i - RD_CL_LHIST);
    else if (i < RD_CL_LASQ) dst = RD_CL_ASUM + (i - RD_CL_LASUM);
    else if (i < RD_CL_LVBA) dst = RD_CL_ASQ + (i - RD_CL_LASQ);
    else if (i < RD_CL_LABA) dst = RD_CL_VBA + (i - RD_CL_LVBA);
    else dst = RD_CL_ABA + (i - RD_CL_LABA);
    atomicAdd(&counts[dst], v);
  }
}

// counts: this threshold's; n_planes: the state's word, or null for every threshold but the first
__global__ void __launch_bounds__(RD_CL_THREADS)
k_cells_planes(int P, const unsigned* __restrict__ plane_words, unsigned long long* __restrict__ counts,
               unsigned long long* __restrict__ n_planes) {
  __shared__ unsigned tab[RD_CL_NKP + RD_CL_NBINS + 1];
  const int tid = threadIdx.x;
  for (int i = tid; i < RD_CL_NKP + RD_CL_NBINS + 1; i += RD_CL_THREADS) tab[i] = 0u;
  __syncthreads();
  const int pl = blockIdx.x * RD_CL_THREADS + tid;
  if (pl < P) {
    const unsigned n = plane_words[pl * 2], amax = plane_words[pl * 2 + 1];
    atomicAdd(&tab[n < RD_CL_NKP - 1 ? n : RD_CL_NKP - 1], 1u);
    atomicAdd(&tab[RD_CL_NKP + (n ? 31 - __builtin_clz(amax) : RD_CL_NBINS)], 1u);
  }
  __syncthreads();
  for (int i = tid; i < RD_CL_NKP + RD_CL_NBINS + 1; i += RD_CL_THREADS)
    if (tab[i]) atomicAdd(&counts[RD_CL_KPP + i], (unsigned long long)tab[i]);      // (largest_area and dry_planes follow cells_per_plane)
  if (n_planes && blockIdx.x == 0 && tid == 0) atomicAdd(n_planes, (unsigned long long)P);
}
