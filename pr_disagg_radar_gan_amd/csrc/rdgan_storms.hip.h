// Storms of hourly fields: wet volumes connected through the day's hours, labelled and counted.
// x [n][24][ny][nx] fp32 with a leading stride day_stride >= 24 ny nx; wet and bad voxels as in rdgan_cells.hip.h.  A voxel of a day
// has the day-local index v = h ny nx + y nx + x.  Two wet voxels of one day are linked when they are neighbours of the same hour
// under the connectivity (the relation of the cells), or lie in consecutive hours h, h + 1 at pixels p, p + d with |dy|, |dx| <=
// reach.  A storm is a maximal set of wet voxels of one day connected by links; its canonical label is its smallest v.
//
// A pass holds D whole days, so the 24 planes of a day are contiguous in the workspace: the maps of rdgan_cells.hip.h over
// [D][24][ny nx] -- vol (uint64), parent (int32), area (uint32, bit 31 the edge flag) -- and one more, last (uint32: the last hour
// of the storm, at its root); then two words per day and the two words per plane the label kernel writes.
//
//  * k_cells_label_tile, k_cells_merge (rdgan_cells.hip.h, unchanged) over the 24 D planes: every plane holds a forest in
//    plane-local indices, and the tile-local roots hold area, edge flag and volume.
//  * k_storm_lift: one thread per voxel adds h ny nx to a parent >= 0.  Both sides of parent[v] <= v move by the same amount, so
//    the invariant holds over the day.  It clears last, and the words of the day.
//  * k_storm_link: one thread per voxel of the hours 0 .. 22 unites it with the wet voxels of the next hour within reach.
//  * k_storm_resolve: one thread per voxel finds its final root and stores it (and the label when asked); a voxel with a non-zero
//    area word that is not the final root hands area, edge flag and volume on to the root's slots, and every voxel with a
//    non-zero area word raises last[root] to its hour.
//  * k_storm_reduce: every final root forms start, last, duration and class and bins its storm into a per-workgroup LDS table,
//    which is merged into the state with 64-bit integer atomics; the storm count and the longest duration of a day are formed
//    with one atomic add and one atomic max per wave.
//  * k_storm_days: one thread per day bins the day's storm count and longest duration.
//
// TERMINATION of link and resolve is the argument of rdgan_cells.hip.h: parent[i] <= i whenever parent[i] >= 0 (the lift keeps
// it), and parent[] only ever decreases (atomicMin in rd_cl_union, and the store of a root found below in resolve).  A find
// descends strictly until it meets a root and ends after at most i steps; a union loop strictly lowers the larger of its two
// indices and ends too, whatever order the hardware picks.  Kernel boundaries are the only ordering between the phases: no
// spin-wait, no grid sync.  No floating-point atomics.  All global offsets are 64-bit; a day-local index fits int32 (a day has at
// most 2^27 voxels, which also leaves bit 31 of the size word to the edge flag and keeps a volume sum below 2^63).
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_cells.hip.h"

#define RD_SM_MAXDAY (1L << 27)          // voxels of a day
#define RD_SM_MAXPASS 2730               // days of one pass: 24 planes each in the label kernel's grid y (65535 / 24)
#define RD_SM_MAXREACH 4
#define RD_SM_NCLASS 4                   // space_edge + 2 time_edge
#define RD_SM_NBINS 28                   // floor(log2(size)) = 0 .. 27
#define RD_SM_NSPD 65                    // storms_per_day[0 .. 64], the last bin open
#define RD_SM_NLONG 25                   // longest_duration[0 .. 24], 0 a day without a wet voxel
#define RD_SM_RCHUNK 4096                // voxels of a day one workgroup of k_storm_reduce takes
#define RD_SM_VOXEL_BYTES 24             // of the workspace: vol 8, parent 4, area 4, last 4, and 4 spare
// the state: counters per threshold, flat
#define RD_SM_WET 0                      // wet_pixels[24]
#define RD_SM_STORMS 24                  // storms[4]
#define RD_SM_DUR 28                     // duration_hist[4][24]
#define RD_SM_START 124                  // start_hour[4][24]
#define RD_SM_HIST 220                   // size_hist[4][28]
#define RD_SM_SSUM 332                   // size_sum[4]
#define RD_SM_SSQ 336                    // size_sq_sum[4]
#define RD_SM_SBD 340                    // size_by_duration[4][24]
#define RD_SM_VBD 436                    // volume_by_duration[4][24]
#define RD_SM_SPD 532                    // storms_per_day[65]
#define RD_SM_LONGEST 597                // longest_duration[25]
#define RD_SM_NC 622
// the LDS table of k_storm_reduce is the state from storms to volume_by_duration, in the same order
#define RD_SM_L(offset) ((offset) - RD_SM_STORMS)
#define RD_SM_NL RD_SM_L(RD_SM_SPD)

// bytes of the workspace for D days of `plane` pixels: the four maps (and the spare word) per voxel, count and longest duration
// per day, then the label kernel's two words per plane
__host__ __device__ inline long rd_sm_ws_bytes(long plane, long D) {
  return D * RD_HOURS * plane * RD_SM_VOXEL_BYTES + D * 8 + D * RD_HOURS * 8;
}

// grid (ceil(V / 256), D), V = 24 plane
__global__ void __launch_bounds__(RD_CL_THREADS)
k_storm_lift(long plane, int* __restrict__ parent_ws, unsigned* __restrict__ last_ws, unsigned* __restrict__ day_words) {
  const long V = RD_HOURS * plane, v = (long)blockIdx.x * RD_CL_THREADS + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 2) day_words[(long)blockIdx.y * 2 + threadIdx.x] = 0u;
  if (v >= V) return;
  const long g = (long)blockIdx.y * V + v;
  const int q = parent_ws[g];
  if (q >= 0) parent_ws[g] = q + (int)(v / plane * plane);
  last_ws[g] = 0u;
}

// grid (ceil(23 plane / 256), D).  In a row of the window of v the thread unites v only with the first wet pixel of every run:
// where b and the pixel left of it are both wet at hour h + 1 and both inside the window, the two are neighbours of one row and
// hour, so k_cells_label_tile or k_cells_merge has put them into one set already (under either connectivity), and THIS thread
// unites v with the left one, or skips it for the one left of that by the same rule: by induction along the run v ends up in
// b's set.  Sets only grow, so the skipped union could change nothing.
__global__ void __launch_bounds__(RD_CL_THREADS)
k_storm_link(int ny, int nx, int reach, int* __restrict__ parent_ws) {
  const long plane = (long)ny * nx, V = RD_HOURS * plane;
  const long v = (long)blockIdx.x * RD_CL_THREADS + threadIdx.x;
  if (v >= V - plane) return;
  int* parent = parent_ws + (long)blockIdx.y * V;
  if (rd_cl_load(parent + v) < 0) return;
  const long p = v % plane;
  const int y = (int)(p / nx), x = (int)(p % nx);
  const long next = v - p + plane;                                         // the first voxel of hour h + 1
  const int ylo = y - reach < 0 ? 0 : y - reach, yhi = y + reach > ny - 1 ? ny - 1 : y + reach;
  const int xlo = x - reach < 0 ? 0 : x - reach, xhi = x + reach > nx - 1 ? nx - 1 : x + reach;
  for (int by = ylo; by <= yhi; ++by) {
    bool left_wet = false;
    for (int bx = xlo; bx <= xhi; ++bx) {
      const long b = next + (long)by * nx + bx;
      const bool wet = rd_cl_load(parent + b) >= 0;
      if (wet && !left_wet) rd_cl_union<false>(parent, (int)v, (int)b);
      left_wet = wet;
    }
  }
}

// grid (ceil(V / 256), D); labels: null, or the map of the whole input, day0 the first day of the pass
__global__ void __launch_bounds__(RD_CL_THREADS)
k_storm_resolve(long plane, long day0, unsigned long long* __restrict__ vol_ws, int* __restrict__ parent_ws,
                unsigned* __restrict__ area_ws, unsigned* __restrict__ last_ws, int* __restrict__ labels) {
  const long V = RD_HOURS * plane, v = (long)blockIdx.x * RD_CL_THREADS + threadIdx.x;
  if (v >= V) return;
  const long base = (long)blockIdx.y * V;
  int* parent = parent_ws + base;
  int r = rd_cl_load(parent + v);
  if (r >= 0) {
    r = rd_cl_find<false>(parent, r);
    // a tile-local root hands its sums on unless it is the final root.  Nobody adds to the slots of one that hands on (only
    // final roots receive), and a final root's slots are read by nobody in this kernel but for the test a != 0 of its own
    // thread, which holds before and after every addition.
    const unsigned a = area_ws[base + v];
    if (a) {
      if (r != (int)v) {
        atomicAdd(&area_ws[base + r], a & ~RD_CL_EDGE);
        if (a & RD_CL_EDGE) atomicOr(&area_ws[base + r], RD_CL_EDGE);
        atomicAdd(&vol_ws[base + r], vol_ws[base + v]);
      }
      atomicMax(&last_ws[base + r], (unsigned)(v / plane));
    }
    // (another thread's find may pass through v meanwhile: it reads the old parent or the root, both above it in its tree)
    __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (labels) labels[(day0 + blockIdx.y) * V + v] = r;
}

// grid (ceil(V / RD_SM_RCHUNK), D); counts: this threshold's
__global__ void __launch_bounds__(RD_CL_THREADS)
k_storm_reduce(long plane, const unsigned long long* __restrict__ vol_ws, const int* __restrict__ parent_ws,
               const unsigned* __restrict__ area_ws, const unsigned* __restrict__ last_ws, unsigned* __restrict__ day_words,
               unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long tab[RD_SM_NL];
  const int tid = threadIdx.x;
  for (int i = tid; i < RD_SM_NL; i += RD_CL_THREADS) tab[i] = 0ull;
  __syncthreads();
  const long V = RD_HOURS * plane, base = (long)blockIdx.y * V, v0 = (long)blockIdx.x * RD_SM_RCHUNK;
  unsigned n = 0, longest = 0;
#pragma unroll 4
  for (int k = 0; k < RD_SM_RCHUNK / RD_CL_THREADS; ++k) {
    const long v = v0 + k * RD_CL_THREADS + tid;
    if (v >= V || parent_ws[base + v] != (int)v) continue;
    const unsigned w = area_ws[base + v], size = w & ~RD_CL_EDGE;          // (a root has size >= 1)
    const unsigned start = (unsigned)(v / plane), last = last_ws[base + v], dur = last - start + 1;
    const int c = (int)(w >> 31) + 2 * (int)(start == 0 || last == RD_HOURS - 1);
    const int b = 31 - __builtin_clz(size), cd = c * RD_HOURS + (int)dur - 1;
    ++n;
    longest = dur > longest ? dur : longest;
    atomicAdd(&tab[RD_SM_L(RD_SM_STORMS) + c], 1ull);
    atomicAdd(&tab[RD_SM_L(RD_SM_DUR) + cd], 1ull);
    atomicAdd(&tab[RD_SM_L(RD_SM_START) + c * RD_HOURS + (int)start], 1ull);
    atomicAdd(&tab[RD_SM_L(RD_SM_HIST) + c * RD_SM_NBINS + b], 1ull);
    atomicAdd(&tab[RD_SM_L(RD_SM_SSUM) + c], (unsigned long long)size);
    atomicAdd(&tab[RD_SM_L(RD_SM_SSQ) + c], (unsigned long long)size * size);
    atomicAdd(&tab[RD_SM_L(RD_SM_SBD) + cd], (unsigned long long)size);
    atomicAdd(&tab[RD_SM_L(RD_SM_VBD) + cd], vol_ws[base + v]);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    n += __shfl_xor(n, s);
    const unsigned o = __shfl_xor(longest, s);
    longest = o > longest ? o : longest;
  }
  if ((tid & 63) == 0 && n) {
    atomicAdd(&day_words[(long)blockIdx.y * 2], n);
    atomicMax(&day_words[(long)blockIdx.y * 2 + 1], longest);
  }
  __syncthreads();
  for (int i = tid; i < RD_SM_NL; i += RD_CL_THREADS)
    if (tab[i]) atomicAdd(&counts[RD_SM_STORMS + i], tab[i]);
}

// counts: this threshold's; n_days: the state's word, or null for every threshold but the first
__global__ void __launch_bounds__(RD_CL_THREADS)
k_storm_days(int D, const unsigned* __restrict__ day_words, unsigned long long* __restrict__ counts,
             unsigned long long* __restrict__ n_days) {
  __shared__ unsigned tab[RD_SM_NSPD + RD_SM_NLONG];
  const int tid = threadIdx.x;
  for (int i = tid; i < RD_SM_NSPD + RD_SM_NLONG; i += RD_CL_THREADS) tab[i] = 0u;
  __syncthreads();
  const int d = blockIdx.x * RD_CL_THREADS + tid;
  if (d < D) {
    const unsigned n = day_words[d * 2], longest = day_words[d * 2 + 1];   // (longest is 0 exactly when n is)
    atomicAdd(&tab[n < RD_SM_NSPD - 1 ? n : RD_SM_NSPD - 1], 1u);
    atomicAdd(&tab[RD_SM_NSPD + longest], 1u);
  }
  __syncthreads();
  for (int i = tid; i < RD_SM_NSPD + RD_SM_NLONG; i += RD_CL_THREADS)
    if (tab[i]) atomicAdd(&counts[RD_SM_SPD + i], (unsigned long long)tab[i]);      // (longest_duration follows storms_per_day)
  if (n_days && blockIdx.x == 0 && tid == 0) atomicAdd(n_days, (unsigned long long)D);
}
