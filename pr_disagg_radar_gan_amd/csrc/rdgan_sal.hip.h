// Object-based verification of hourly fields: the per-plane records from which SAL (Wernli et al. 2008) is
// formed -- structure S, amplitude A, location L = L1 + L2 of a generated plane against the observed one.
// x [n][24][ny][nx] fp32 as the cells read it (rdgan_cells.hip.h): a plane is one (i, h), a pixel is bad when NaN or +-inf, wet at
// threshold t when finite and x > thr[t]; the objects of a plane ARE its cells, labelled by rd_cl_label_planes and k_cells_resolve.
// The mass of a valid pixel is q = rd_depth_q(clamp(x, 0, RD_DEPTH_MAX - 1 / RD_DEPTH_UNIT)), 0 <= q < 2^21, in 1/1024 mm.
//
// Per plane (threshold-independent, int64): n_bad, M0 = sum q, Mx = sum q x, My = sum q y over the valid pixels.
// Per plane and threshold: n_objects, n_wet, R = sum_n R_n (int64) and, in fp64,
//   V = (sum_n R_n (R_n / Rmax_n)) / R          r = (sum_n R_n hypot(Sx_n / R_n - Mx / M0, Sy_n / R_n - My / M0)) / R
// with R_n = sum q, Rmax_n = max q, Sx_n = sum q x, Sy_n = sum q y over the pixels of object n.  An object with R_n = 0 (every
// pixel below 1/2048 mm) adds nothing to either sum; V = r = 0 when R = 0, so also without an object.
//
// OVERFLOW: the largest sum is Sx or Mx <= (2^21 - 1) (max(ny, nx) - 1) ny nx.  The entries refuse a plane with
// 2^21 max(ny, nx) ny nx >= 2^63, i.e. max(ny, nx) ny nx >= 2^42 (rd_sal_shape_ok), so every sum stays below 2^63.
//
// The workspace holds, for the P planes of a pass, the three maps of the cells (16 bytes per pixel), the object map obj
// [P][ny nx][4] u64 = (R, Rmax, Sx, Sy) at the root's pixel (32 bytes per pixel), 5 words per (plane, chunk of 4096 pixels), the
// cells' two words per plane and 24 words per plane that take the label kernel's wet counts, which nobody reads.
//
//  * k_sal_clear: after resolve; every final root (parent[p] == p) zeroes its own four words.  Nothing else of obj is ever read.
//  * k_sal_moments: one thread per pixel in flat order.  Lanes that follow each other with the same root (the pixels of a row run
//    do) are summed inside the wave by a segmented reduction, and the first lane of each segment adds R, Sx, Sy and takes the max
//    into the root's words: one 64-bit integer atomic per run segment and quantity.  For the first threshold the whole-plane sums
//    are reduced per workgroup and added with one atomic per workgroup and quantity.
//  * k_sal_plane: one workgroup per chunk of RD_SAL_CHUNK pixels.  Thread i takes the roots among pixels chunk 4096 + 256 k + i,
//    k = 0 .. 15 in this order, the 64 lanes are folded by a butterfly, the four waves in order: the tree is fixed by the pixel
//    index alone.  -> the chunk's (n_objects, n_wet, R, sum_V, sum_r).
//  * k_sal_final: one wave per plane folds the chunks (lane i takes chunks i, i + 64, ... in order, then the butterfly) and writes
//    the record.  The chunking is a function of ny nx only, so V and r of a plane are bitwise the same under any grouping of the
//    planes into passes or calls.
// No floating-point atomics, no spin-wait, no grid sync; kernel boundaries order the phases.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_cells.hip.h"

#define RD_SAL_THREADS 256
#define RD_SAL_CHUNK 4096                 // pixels of a plane one workgroup of k_sal_plane takes
#define RD_SAL_NPART 5                    // words of a chunk: n_objects, n_wet, R (u64), sum_V, sum_r (fp64)
#define RD_SAL_SINK 24                    // words per plane behind the partials: the label kernel's wet counts land there
#define RD_SAL_MAXMOMENT (1LL << 42)      // max(ny, nx) ny nx stays below this

static_assert((long)RD_DEPTH_MAX * RD_DEPTH_UNIT == (1L << 21), "q < 2^21 is what the overflow bound of the moments assumes");
static_assert(RD_SAL_CHUNK % RD_SAL_THREADS == 0, "every thread of k_sal_plane takes the same number of pixels");

__host__ __device__ inline long rd_sal_chunks(long plane) { return (plane + RD_SAL_CHUNK - 1) / RD_SAL_CHUNK; }
// bytes of the workspace for P planes of `plane` pixels: the cells' maps and words, obj, the chunk partials, the sink
__host__ __device__ inline long rd_sal_ws_bytes(long plane, long P) {
  return rd_cl_ws_bytes(plane, P) + P * (plane * 32 + rd_sal_chunks(plane) * RD_SAL_NPART * 8 + RD_SAL_SINK * 8);
}

// the mass of a finite value: clamped into the depth range, then the shared fixed point
__device__ __forceinline__ unsigned long long rd_sal_q(float v) {
  const float hi = (float)RD_DEPTH_MAX - 1.0f / (float)RD_DEPTH_UNIT;      // 2047.9990234375, exact in fp32
  return (unsigned long long)rd_depth_q(fminf(fmaxf(v, 0.0f), hi));
}

__global__ void __launch_bounds__(RD_SAL_THREADS)
k_sal_clear(long plane, const int* __restrict__ parent_ws, unsigned long long* __restrict__ obj) {
  const long p = (long)blockIdx.x * RD_SAL_THREADS + threadIdx.x;
  if (p >= plane) return;
  const long g = (long)blockIdx.y * plane + p;
  if (parent_ws[g] != (int)p) return;
  ulonglong2* o = reinterpret_cast<ulonglong2*>(obj + g * 4);
  o[0] = make_ulonglong2(0ull, 0ull);
  o[1] = make_ulonglong2(0ull, 0ull);
}

__global__ void __launch_bounds__(RD_SAL_THREADS)
k_sal_moments(const float* __restrict__ x, long day_stride, int nx, long plane, long plane0, int first,
              const int* __restrict__ parent_ws, unsigned long long* __restrict__ obj, unsigned long long* __restrict__ plane_out) {
  __shared__ unsigned long long wsum[RD_SAL_THREADS / 64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p = (long)blockIdx.x * RD_SAL_THREADS + tid;
  const long pl = blockIdx.y, gp = plane0 + pl, base = pl * plane;
  const float* src = x + (gp / RD_HOURS) * day_stride + (gp % RD_HOURS) * plane;
  const bool in = p < plane;
  float v = 0.0f;
  int root = -1;
  if (in) {
    v = src[p];
    root = parent_ws[base + p];
  }
  const bool bad = rd_nonfinite(v);                                        // (a lane outside the plane holds 0: valid, mass 0)
  const unsigned long long q = bad ? 0ull : rd_sal_q(v);
  const int ip = in ? (int)p : 0, py = ip / nx, px = ip - py * nx;
  const unsigned long long qx = q * (unsigned long long)px, qy = q * (unsigned long long)py;

  // the objects: lanes that follow each other with one root are one segment; after the steps its first lane holds its sums.
  // A wave without a wet pixel (most are, in rain) skips all of it; the sum of q over 64 lanes and its max fit 32 bits.
  if (__ballot(root >= 0)) {
    const int prev = __shfl_up(root, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != root);
    const unsigned long long after = (heads >> lane) >> 1;                 // bit j: lane + 1 + j starts a segment
    unsigned sq = (unsigned)q, sm = (unsigned)q;
    unsigned long long sx = qx, sy = qy;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned oq = __shfl_down(sq, d), om = __shfl_down(sm, d);
      const unsigned long long ox = __shfl_down(sx, d), oy = __shfl_down(sy, d);
      if (lane + d < 64 && !(after & ((1ull << d) - 1ull))) {              // lane + d lies in this lane's segment
        sq += oq;
        sx += ox;
        sy += oy;
        sm = om > sm ? om : sm;
      }
    }
    if (root >= 0 && ((heads >> lane) & 1ull)) {
      unsigned long long* o = obj + (base + root) * 4;
      atomicAdd(o + 0, (unsigned long long)sq);
      atomicMax(o + 1, (unsigned long long)sm);
      atomicAdd(o + 2, sx);
      atomicAdd(o + 3, sy);
    }
  }

  if (!first) return;                                                      // (uniform: the whole-plane sums do not depend on t)
  unsigned long long a0 = bad ? 1ull : 0ull, a1 = q, a2 = qx, a3 = qy;
  if (__ballot(bad || q)) {                                                // (a wave of zeros has its sums already)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      a0 += __shfl_xor(a0, s);
      a1 += __shfl_xor(a1, s);
      a2 += __shfl_xor(a2, s);
      a3 += __shfl_xor(a3, s);
    }
  }
  if (lane == 0) {
    wsum[wave][0] = a0;
    wsum[wave][1] = a1;
    wsum[wave][2] = a2;
    wsum[wave][3] = a3;
  }
  __syncthreads();
  if (tid < 4) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int w = 0; w < RD_SAL_THREADS / 64; ++w) s += wsum[w][tid];
    if (s) atomicAdd(&plane_out[gp * 4 + tid], s);                         // (n_bad, M0, Mx, My)
  }
}

// the butterfly both reductions use: every lane ends with the same value, a + b and b + a being the same fp64
__device__ __forceinline__ void rd_sal_fold(unsigned long long& n, unsigned long long& w, unsigned long long& R, double& v, double& r) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    n += __shfl_xor(n, s);
    w += __shfl_xor(w, s);
    R += __shfl_xor(R, s);
    v += __shfl_xor(v, s);
    r += __shfl_xor(r, s);
  }
}

__global__ void __launch_bounds__(RD_SAL_THREADS)
k_sal_plane(long plane, long plane0, const int* __restrict__ parent_ws, const unsigned* __restrict__ area_ws,
            const unsigned long long* __restrict__ obj, const unsigned long long* __restrict__ plane_out,
            unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long li[RD_SAL_THREADS / 64][3];
  __shared__ double lf[RD_SAL_THREADS / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long pl = blockIdx.y, gp = plane0 + pl, base = pl * plane, p0 = (long)blockIdx.x * RD_SAL_CHUNK;
  const unsigned long long M0 = plane_out[gp * 4 + 1];
  // the centre of mass of the whole field (M0 = 0 leaves every object without mass: the centre is then never used)
  const double cx = M0 ? (double)plane_out[gp * 4 + 2] / (double)M0 : 0.0, cy = M0 ? (double)plane_out[gp * 4 + 3] / (double)M0 : 0.0;
  unsigned long long n = 0ull, w = 0ull, R = 0ull;
  double v = 0.0, r = 0.0;
  for (int k = 0; k < RD_SAL_CHUNK / RD_SAL_THREADS; ++k) {
    const long p = p0 + k * RD_SAL_THREADS + tid;
    if (p >= plane || parent_ws[base + p] != (int)p) continue;
    const ulonglong2* o = reinterpret_cast<const ulonglong2*>(obj + (base + p) * 4);
    const ulonglong2 a = o[0], b = o[1];                                   // (R_n, Rmax_n), (Sx_n, Sy_n)
    ++n;
    w += (unsigned long long)(area_ws[base + p] & ~RD_CL_EDGE);
    R += a.x;
    if (a.x) {
      const double Rn = (double)a.x;
      v += Rn * (Rn / (double)a.y);
      r += Rn * hypot((double)b.x / Rn - cx, (double)b.y / Rn - cy);
    }
  }
  rd_sal_fold(n, w, R, v, r);
  if (lane == 0) {
    li[wave][0] = n;
    li[wave][1] = w;
    li[wave][2] = R;
    lf[wave][0] = v;
    lf[wave][1] = r;
  }
  __syncthreads();
  if (tid == 0) {
    n = w = R = 0ull;
    v = r = 0.0;
    for (int i = 0; i < RD_SAL_THREADS / 64; ++i) {
      n += li[i][0];
      w += li[i][1];
      R += li[i][2];
      v += lf[i][0];
      r += lf[i][1];
    }
    unsigned long long* out = partial + (pl * gridDim.x + blockIdx.x) * RD_SAL_NPART;
    out[0] = n;
    out[1] = w;
    out[2] = R;
    out[3] = (unsigned long long)__double_as_longlong(v);
    out[4] = (unsigned long long)__double_as_longlong(r);
  }
}

// one wave per plane
__global__ void __launch_bounds__(64)
k_sal_final(long chunks, long plane0, int t, int T, const unsigned long long* __restrict__ partial, long long* __restrict__ obj_out,
            double* __restrict__ vr_out) {
  const int lane = threadIdx.x;
  const long pl = blockIdx.x, gp = plane0 + pl;
  unsigned long long n = 0ull, w = 0ull, R = 0ull;
  double v = 0.0, r = 0.0;
  for (long c = lane; c < chunks; c += 64) {
    const unsigned long long* in = partial + (pl * chunks + c) * RD_SAL_NPART;
    n += in[0];
    w += in[1];
    R += in[2];
    v += __longlong_as_double((long long)in[3]);
    r += __longlong_as_double((long long)in[4]);
  }
  rd_sal_fold(n, w, R, v, r);
  if (lane == 0) {
    long long* o = obj_out + (gp * T + t) * 3;
    o[0] = (long long)n;
    o[1] = (long long)w;
    o[2] = (long long)R;
    double* f = vr_out + (gp * T + t) * 2;
    f[0] = R ? v / (double)R : 0.0;
    f[1] = R ? r / (double)R : 0.0;
  }
}
