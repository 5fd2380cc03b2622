// Verification of field ensembles against observed hours: rank histogram, Brier sums with the reliability
// table, fractions skill score.  Positions p < P are laid out ([D,] 24, ny, nx): hour(p) = (p / (ny nx)) % 24.
//
//  * k_verify_accumulate: members x[s * member_stride + p], s < n, and the observation o[p] -> the state, ADDED to what is there:
//      exceed[t][p] += #{s : x_s[p] > thr[t]},  below[p] += #{s : x_s[p] < o[p]},  equal[p] += #{s : x_s[p] == o[p]}   (int32)
//      bad[p] |= o[p] is NaN or a member is NaN at p                                                                 (uint8)
//    fp32 IEEE comparisons, so a NaN counts nowhere.  A thread owns V adjacent positions (V = 4: 16-byte loads of members, observation
//    and state; V = 1: the scalar path for a stride, a P or a pointer that does not allow them), loops over the members of the call
//    with the T + 2 counters of each position in registers, and touches the state once.  The ensemble is read exactly once.
//  * k_verify_reduce: one pass over state and observation -> rank_hist [24][S + 1], reliability [T][24][n_bins][3] = (count, sum e,
//    sum c), brier [T][24][4] = (N, sum e, sum c e, sum c^2), 64-bit integers, over the valid (bad == 0) positions:
//      rank = below + ((b24 (equal + 1)) >> 24),  b24 = rd_bits(rd_member_key(key, p), 0) >> 8: ties broken by a hash of the position
//      c = exceed[t][p], e = o > thr[t], bin = (c n_bins) / (S + 1)
//    blockIdx.y is the hour, so a workgroup keeps ONE hour's histograms in LDS (S + 1 + 3 T n_bins counters of 32 bits, at most 256
//    chunks of 2048 positions: no counter passes 2^31) and merges them once with 64-bit integer atomics; the Brier sums ride in
//    registers.  Integer sums do not depend on the order, so two calls agree exactly.
//  * FSS, per day: k_verify_fss_rows forms C = exceed[t] and E = [o > thr[t]] (0 at a bad position) for the 24 T planes of the day
//    and scans them along x (one wave per row); k_verify_fss_cols scans along y, giving summed-area tables in uint32 (box sums stay
//    below 2^26 <= 2^32, so differences taken modulo 2^32 are exact); k_verify_fss_box takes four reads per table, box and pixel --
//    the cost does not grow with w^2 -- and adds (BC - S BE)^2 and BC^2 + (S BE)^2 in fp64 per thread, then a fixed tree per
//    workgroup; k_verify_fss_final adds the workgroups' partials in order onto the output.  No floating-point atomics.
// All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_rng.h"
#include "rdgan_hourly.hip.h"

#define RD_VF_MAXT RD_THR_MAX
#define RD_VF_MAXW 8
#define RD_VF_MAXS 4096
#define RD_VF_MAXBINS 64
#define RD_VF_THREADS 256
#define RD_VF_CHUNK 2048                 // positions of one (day, hour) plane a workgroup of k_verify_reduce takes at a time
#define RD_VF_MAXUNITS 256               // chunks per workgroup at most: 2^19 positions, sum c <= 2^31 in a 32-bit LDS counter
#define RD_VF_BOX_MAXBLOCKS 128          // workgroups of k_verify_fss_box per plane

struct rd_vf_widths {
  int v[RD_VF_MAXW];
};

template <int V> __device__ __forceinline__ void rd_vf_add(int* __restrict__ p, const int (&a)[V]) {
  if constexpr (V == 4) {
    int4 q = *reinterpret_cast<const int4*>(p);
    q.x += a[0]; q.y += a[1]; q.z += a[2]; q.w += a[3];
    *reinterpret_cast<int4*>(p) = q;
  } else {
    *p += a[0];
  }
}

template <int T, int V>
__global__ void __launch_bounds__(RD_VF_THREADS)
k_verify_accumulate(const float* __restrict__ x, long member_stride, int n, long P, const float* __restrict__ obs, rd_thr thr,
                    int* __restrict__ exceed, int* __restrict__ below, int* __restrict__ equal, unsigned char* __restrict__ bad) {
  const long groups = P / V;                                              // (V = 4 is chosen only for P % 4 == 0)
  for (long g = (long)blockIdx.x * RD_VF_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * RD_VF_THREADS) {
    const long p = g * V;
    float o[V];
    rd_load<V>(obs + p, o);
    int ex[T][V], bl[V], eq[V], nn[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      bl[j] = 0;
      eq[j] = 0;
      nn[j] = o[j] != o[j];
#pragma unroll
      for (int t = 0; t < T; ++t) ex[t][j] = 0;
    }
    const float* src = x + p;
#pragma unroll 4
    for (int s = 0; s < n; ++s) {
      float v[V];
      rd_load<V>(src + (long)s * member_stride, v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        bl[j] += v[j] < o[j];
        eq[j] += v[j] == o[j];
        nn[j] |= v[j] != v[j];
#pragma unroll
        for (int t = 0; t < T; ++t) ex[t][j] += v[j] > thr.v[t];
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) rd_vf_add<V>(exceed + (long)t * P + p, ex[t]);
    rd_vf_add<V>(below + p, bl);
    rd_vf_add<V>(equal + p, eq);
    if constexpr (V == 4) {
      const unsigned m = (nn[0] ? 1u : 0u) | (nn[1] ? 0x100u : 0u) | (nn[2] ? 0x10000u : 0u) | (nn[3] ? 0x1000000u : 0u);
      if (m) *reinterpret_cast<unsigned*>(bad + p) |= m;
    } else {
      if (nn[0]) bad[p] = 1;
    }
  }
}

// grid (nbx, 24); dynamic LDS 4 T 8-byte Brier slots, then 3 T n_bins + S + 1 32-bit counters.  The three outputs are cleared by the
// caller.  A state that does not fit S (a count above S: the caller's error) is clamped, so nothing is written out of bounds.
__global__ void __launch_bounds__(RD_VF_THREADS)
k_verify_reduce(const float* __restrict__ obs, const int* __restrict__ exceed, const int* __restrict__ below,
                const int* __restrict__ equal, const unsigned char* __restrict__ bad, long P, long plane, long n_planes, int S, int T,
                rd_thr thr, int n_bins, uint32_t key, unsigned long long* __restrict__ rank_hist,
                unsigned long long* __restrict__ reliability, unsigned long long* __restrict__ brier) {
  extern __shared__ unsigned long long rd_vf_lds[];
  unsigned long long* bs = rd_vf_lds;                                      // [T][4]
  unsigned* rel = reinterpret_cast<unsigned*>(bs + RD_VF_MAXT * 4);        // [T][n_bins][3]
  unsigned* rh = rel + T * n_bins * 3;                                     // [S + 1]
  const int tid = threadIdx.x, hour = blockIdx.y;
  const int n_rel = T * n_bins * 3;
  for (int i = tid; i < RD_VF_MAXT * 4; i += RD_VF_THREADS) bs[i] = 0ull;
  for (int i = tid; i < n_rel + S + 1; i += RD_VF_THREADS) rel[i] = 0u;
  __syncthreads();
  // the planes of this hour are q = hour, hour + 24, ..: the last day may stop short of 24 hours
  const long chunks = (plane + RD_VF_CHUNK - 1) / RD_VF_CHUNK, units = ((n_planes + RD_HOURS - 1) / RD_HOURS) * chunks;
  unsigned n_valid = 0, se[RD_VF_MAXT], sce[RD_VF_MAXT];
  unsigned long long sc2[RD_VF_MAXT];
#pragma unroll
  for (int t = 0; t < RD_VF_MAXT; ++t) {
    se[t] = 0;
    sce[t] = 0;
    sc2[t] = 0;
  }
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long q = (u / chunks) * RD_HOURS + hour;
    if (q >= n_planes) continue;
    const long base = q * plane;
    const long i0 = (u % chunks) * RD_VF_CHUNK, i1 = i0 + RD_VF_CHUNK < plane ? i0 + RD_VF_CHUNK : plane;
    for (long i = i0 + tid; i < i1; i += RD_VF_THREADS) {
      const long p = base + i;
      const float o = obs[p];
      if (bad[p] || o != o) continue;
      ++n_valid;
      const uint32_t b24 = rd_bits(rd_member_key(key, (uint64_t)p), 0u) >> 8;
      long r = (long)below[p] + (long)(((unsigned long long)b24 * (unsigned long long)((long)equal[p] + 1)) >> 24);
      r = r < 0 ? 0 : (r > S ? S : r);
      atomicAdd(&rh[r], 1u);
#pragma unroll
      for (int t = 0; t < RD_VF_MAXT; ++t)
        if (t < T) {
          int c = exceed[(long)t * P + p];
          c = c < 0 ? 0 : (c > S ? S : c);
          const unsigned e = o > thr.v[t] ? 1u : 0u;
          unsigned* cell = rel + (t * n_bins + (c * n_bins) / (S + 1)) * 3;
          atomicAdd(cell, 1u);
          if (e) atomicAdd(cell + 1, 1u);
          if (c) atomicAdd(cell + 2, (unsigned)c);
          se[t] += e;
          sce[t] += e ? (unsigned)c : 0u;
          sc2[t] += (unsigned long long)((long)c * c);
        }
    }
  }
#pragma unroll
  for (int t = 0; t < RD_VF_MAXT; ++t)
    if (t < T && n_valid) {
      atomicAdd(&bs[t * 4 + 0], (unsigned long long)n_valid);
      if (se[t]) atomicAdd(&bs[t * 4 + 1], (unsigned long long)se[t]);
      if (sce[t]) atomicAdd(&bs[t * 4 + 2], (unsigned long long)sce[t]);
      if (sc2[t]) atomicAdd(&bs[t * 4 + 3], sc2[t]);
    }
  __syncthreads();
  for (int i = tid; i <= S; i += RD_VF_THREADS)
    if (rh[i]) atomicAdd(&rank_hist[(long)hour * (S + 1) + i], (unsigned long long)rh[i]);
  for (int i = tid; i < n_rel; i += RD_VF_THREADS)
    if (rel[i]) {
      const int t = i / (n_bins * 3), rest = i % (n_bins * 3);
      atomicAdd(&reliability[((long)t * RD_HOURS + hour) * n_bins * 3 + rest], (unsigned long long)rel[i]);
    }
  for (int i = tid; i < T * 4; i += RD_VF_THREADS)
    if (bs[i]) atomicAdd(&brier[((long)(i >> 2) * RD_HOURS + hour) * 4 + (i & 3)], bs[i]);
}

// ------------------------------------------------------------------------------------------------------------------------------
// FSS.  Workspace planes of one day: q = hour * T + t, satC / satE [24 T][ny][nx] uint32.
// One wave per row (a workgroup takes 4): the inclusive scan of 64 values by shuffles, a carry from segment to segment.
__global__ void __launch_bounds__(RD_VF_THREADS)
k_verify_fss_rows(const float* __restrict__ obs, const int* __restrict__ exceed, const unsigned char* __restrict__ bad, long P,
                  long day, int ny, int nx, int S, int T, rd_thr thr, unsigned* __restrict__ satC, unsigned* __restrict__ satE) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (RD_VF_THREADS / 64) + (threadIdx.x >> 6);      // the same in all lanes of a wave
  if (row >= (long)RD_HOURS * T * ny) return;
  const int y = (int)(row % ny);
  const long q = row / ny;
  const int t = (int)(q % T), hour = (int)(q / T);
  float th = thr.v[0];
#pragma unroll
  for (int k = 1; k < RD_VF_MAXT; ++k) th = k == t ? thr.v[k] : th;
  const long src = ((day * RD_HOURS + hour) * ny + y) * (long)nx, dst = row * (long)nx;
  const int* ex = exceed + (long)t * P + src;
  unsigned carry_c = 0, carry_e = 0;
  for (int x0 = 0; x0 < nx; x0 += 64) {
    const int x = x0 + lane;
    unsigned c = 0, e = 0;
    if (x < nx) {
      const float o = obs[src + x];
      if (!bad[src + x] && o == o) {
        const int cx = ex[x];
        c = (unsigned)(cx < 0 ? 0 : (cx > S ? S : cx));          // (a count above S: clamped as in k_verify_reduce)
        e = o > th ? 1u : 0u;
      }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned uc = __shfl_up(c, off, 64), ue = __shfl_up(e, off, 64);
      if (lane >= off) {
        c += uc;
        e += ue;
      }
    }
    c += carry_c;
    e += carry_e;
    if (x < nx) {
      satC[dst + x] = c;
      satE[dst + x] = e;
    }
    carry_c = __shfl(c, 63, 64);
    carry_e = __shfl(e, 63, 64);
  }
}

// a thread per (plane, x) walks down y: a wave reads and writes 64 adjacent columns of a row
__global__ void __launch_bounds__(RD_VF_THREADS)
k_verify_fss_cols(unsigned* __restrict__ satC, unsigned* __restrict__ satE, long planes, int ny, int nx) {
  const long i = (long)blockIdx.x * RD_VF_THREADS + threadIdx.x;
  if (i >= planes * nx) return;
  const long at = (i / nx) * (long)ny * nx + (i % nx);
  unsigned c = 0, e = 0;
  for (int y = 0; y < ny; ++y) {
    const long a = at + (long)y * nx;
    c += satC[a];
    e += satE[a];
    satC[a] = c;
    satE[a] = e;
  }
}

// the sum over rows y0 .. y1 and columns x0 .. x1 of the plane whose summed-area table is `sat`, modulo 2^32
__device__ __forceinline__ unsigned rd_vf_box(const unsigned* __restrict__ sat, int nx, int y0, int y1, int x0, int x1) {
  const unsigned* hi = sat + (long)y1 * nx;
  unsigned s = hi[x1];
  if (x0 > 0) s -= hi[x0 - 1];
  if (y0 > 0) {
    const unsigned* lo = sat + (long)(y0 - 1) * nx;
    s -= lo[x1];
    if (x0 > 0) s += lo[x0 - 1];
  }
  return s;
}

// grid (nblk, 24 T); partial [24 T][nblk][W][2] doubles = (num, den) of the workgroup's pixels
__global__ void __launch_bounds__(RD_VF_THREADS)
k_verify_fss_box(const unsigned* __restrict__ satC, const unsigned* __restrict__ satE, int ny, int nx, int S, rd_vf_widths wd, int W,
                 double* __restrict__ partial) {
  __shared__ double red[RD_VF_THREADS];
  const int tid = threadIdx.x;
  const long plane = (long)ny * nx, q = blockIdx.y;
  const unsigned* sc = satC + q * plane;
  const unsigned* se = satE + q * plane;
  double num[RD_VF_MAXW], den[RD_VF_MAXW];
#pragma unroll
  for (int i = 0; i < RD_VF_MAXW; ++i) {
    num[i] = 0.0;
    den[i] = 0.0;
  }
  for (long pix = (long)blockIdx.x * RD_VF_THREADS + tid; pix < plane; pix += (long)gridDim.x * RD_VF_THREADS) {
    const int y = (int)(pix / nx), x = (int)(pix % nx);
#pragma unroll
    for (int i = 0; i < RD_VF_MAXW; ++i)
      if (i < W) {
        const int r = wd.v[i] >> 1;
        const int y0 = y - r > 0 ? y - r : 0, y1 = y + r < ny - 1 ? y + r : ny - 1;
        const int x0 = x - r > 0 ? x - r : 0, x1 = x + r < nx - 1 ? x + r : nx - 1;
        const long bc = (long)rd_vf_box(sc, nx, y0, y1, x0, x1), be = (long)S * (long)rd_vf_box(se, nx, y0, y1, x0, x1);
        num[i] += (double)((bc - be) * (bc - be));
        den[i] += (double)(bc * bc + be * be);
      }
  }
  double* out = partial + (q * gridDim.x + blockIdx.x) * (long)W * 2;
#pragma unroll
  for (int i = 0; i < RD_VF_MAXW; ++i)
    if (i < W) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        __syncthreads();
        red[tid] = k ? den[i] : num[i];
        __syncthreads();
        for (int h = RD_VF_THREADS >> 1; h > 0; h >>= 1) {
          if (tid < h) red[tid] += red[tid + h];
          __syncthreads();
        }
        if (tid == 0) out[i * 2 + k] = red[0];
      }
    }
}

// one thread per (plane q = hour * T + t, width i): the nblk partials in order, added onto fss_sums [T][W][24][2]
__global__ void __launch_bounds__(RD_VF_THREADS)
k_verify_fss_final(const double* __restrict__ partial, int nblk, int T, int W, double* __restrict__ fss_sums) {
  const int j = blockIdx.x * RD_VF_THREADS + threadIdx.x;
  if (j >= RD_HOURS * T * W) return;
  const int i = j % W, q = j / W, t = q % T, hour = q / T;
  double num = 0.0, den = 0.0;
  for (int b = 0; b < nblk; ++b) {
    const double* src = partial + ((long)q * nblk + b) * W * 2 + i * 2;
    num += src[0];
    den += src[1];
  }
  double* dst = fss_sums + (((long)t * W + i) * RD_HOURS + hour) * 2;
  dst[0] += num;
  dst[1] += den;
}
