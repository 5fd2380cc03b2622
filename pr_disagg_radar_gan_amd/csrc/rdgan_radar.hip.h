// Training set from raw radar frames: the two host scripts in front of everything else in the reference.
//  * k_radar_hourly: convert_smhi_radardata.py:38-44 (uint8 radar code -> mm per frame; 255 = missing -> NaN) as a 256-entry table
//    built on the host, and reformat_data.py:72-91 (sum the frames of an hour with skipna=False, reshape to (days, 24, ny, nx)).
//    The daily-sum plane the valid-tile scan needs falls out of the same pass, as does the count of missing pixel-hours.
//  * k_valid_tiles_daily: the box test of compute_valid_indices.py:83-91 on that plane (1 float per pixel instead of 24).
//  * k_daily_sum: the plane for an hourly array that did not come from k_radar_hourly.
// Every sum is sequential fp32 in the order the numpy restatement (tests/radar_np.py) states, so results match bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RD_RADAR_THREADS 256

template <int W> struct RdCodes;
template <> struct RdCodes<16> { typedef uint4 type; };
template <> struct RdCodes<4> { typedef uint32_t type; };
template <> struct RdCodes<1> { typedef unsigned char type; };

// code number i (memory order, little endian) of a group of W codes
template <int W> __device__ __forceinline__ unsigned rd_code(const typename RdCodes<W>::type& v, int i);
template <> __device__ __forceinline__ unsigned rd_code<16>(const uint4& v, int i) {
  const uint32_t w = i < 4 ? v.x : i < 8 ? v.y : i < 12 ? v.z : v.w;
  return (w >> (8 * (i & 3))) & 0xffu;
}
template <> __device__ __forceinline__ unsigned rd_code<4>(const uint32_t& v, int i) { return (v >> (8 * i)) & 0xffu; }
template <> __device__ __forceinline__ unsigned rd_code<1>(const unsigned char& v, int) { return v; }

template <int W> __device__ __forceinline__ void rd_store_group(float* p, const float* v) {
  if constexpr (W == 1) {
    p[0] = v[0];
  } else {
#pragma unroll
    for (int q = 0; q < W / 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  }
}

// One lane per (day, group of W consecutive pixels of the flat ny*nx plane): it walks the day's 24 * FPH frames in order, so the hour
// sums feed the daily sum in registers.  The FPH loads of an hour (W bytes each, 16 B = one dwordx4 at W = 16) are issued together;
// a wave keeps FPH * 64 * W bytes in flight.  lut: 256 floats staged once per workgroup into LDS (1 KB); a lookup is one ds_read_b32
// at a data-dependent address (equal codes in a wave broadcast, codes 64 apart share a bank).
//   hourly[d,h,p] = ((lut[c0] + lut[c1]) + lut[c2]) + ...     in frame order
//   daily[d,p]    = ((hourly[d,0,p] + hourly[d,1,p]) + ...)   over h = 0..23, of the rounded hourly values
//   *missing     += number of NaN hourly values              (per-wave sums, one 64-bit atomic per workgroup)
// W = 16 / 4 need group-aligned pointers and plane % W == 0 (the host picks); plane_groups = ceil(plane / W).
template <int W, int FPH>
__global__ void __launch_bounds__(RD_RADAR_THREADS)
k_radar_hourly(const unsigned char* __restrict__ codes, const float* __restrict__ lut, long n_days, long plane, long plane_groups,
               float* __restrict__ hourly, float* __restrict__ daily, unsigned long long* __restrict__ missing) {
  typedef typename RdCodes<W>::type codes_t;
  __shared__ float s_lut[256];
  __shared__ unsigned s_miss[RD_RADAR_THREADS / 64];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  unsigned n_miss = 0;
  const long total = n_days * plane_groups;
  for (long f = blockIdx.x * (long)RD_RADAR_THREADS + threadIdx.x; f < total; f += (long)gridDim.x * RD_RADAR_THREADS) {
    const long d = f / plane_groups, p0 = (f - d * plane_groups) * W;
    const unsigned char* src = codes + d * (24L * FPH) * plane + p0;
    float* dst = hourly + d * 24L * plane + p0;
    float day[W];
#pragma unroll
    for (int i = 0; i < W; ++i) day[i] = 0.f;                 // (0 + x = x: the order of k_gather_tiles' own daily sum)
#pragma unroll 1
    for (int h = 0; h < 24; ++h) {
      codes_t c[FPH];
#pragma unroll
      for (int k = 0; k < FPH; ++k) c[k] = *reinterpret_cast<const codes_t*>(src + (long)(h * FPH + k) * plane);
      float acc[W];
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = s_lut[rd_code<W>(c[0], i)];
#pragma unroll
      for (int k = 1; k < FPH; ++k)
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = acc[i] + s_lut[rd_code<W>(c[k], i)];
#pragma unroll
      for (int i = 0; i < W; ++i) {
        n_miss += acc[i] != acc[i];
        day[i] = day[i] + acc[i];
      }
      rd_store_group<W>(dst + h * plane, acc);
    }
    if (daily) rd_store_group<W>(daily + d * plane + p0, day);
  }
  if (missing) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_miss += __shfl_down(n_miss, off, 64);
    if ((threadIdx.x & 63) == 0) s_miss[threadIdx.x >> 6] = n_miss;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < RD_RADAR_THREADS / 64; ++w) t += s_miss[w];
      if (t) atomicAdd(missing, t);
    }
  }
}

// daily[d,p] = sequential fp32 sum over the 24 hours (np.sum(data[d], axis=0), and the order of k_gather_tiles / k_valid_tiles)
__global__ void k_daily_sum(const float* __restrict__ hourly, long n_days, long plane, float* __restrict__ daily) {
  const long total = n_days * plane;
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < total; f += (long)gridDim.x * blockDim.x) {
    const long d = f / plane;
    const float* p = hourly + d * 23L * plane + f;          // (d * 24 * plane + (f - d * plane))
    float sum = 0.f;
    for (int h = 0; h < 24; ++h) sum += p[h * plane];
    daily[f] = sum;
  }
}

// One wave per (day, box row, box column) of the stride grid, four boxes per 256-thread block: the lanes sweep the nd x nd box of
// the daily plane, the verdict is two wave-wide votes (no LDS, no barrier).  valid[...] = 1 if the box holds no NaN and at least
// n_thresh points above thresh, else 0 -- the counts are integers, so the order of the sweep does not matter.
__global__ void __launch_bounds__(256)
k_valid_tiles_daily(const float* __restrict__ daily, long n_boxes, int ny, int nx, int nd, int stride, int nbi, int nbj, float thresh,
                    int n_thresh, int* __restrict__ valid) {
  const int lane = threadIdx.x & 63;
  const long plane = (long)ny * nx;
  for (long b = blockIdx.x * 4L + (threadIdx.x >> 6); b < n_boxes; b += gridDim.x * 4L) {
    const int bj = (int)(b % nbj), bi = (int)((b / nbj) % nbi);
    const long t = b / ((long)nbj * nbi);
    const float* p = daily + t * plane + (long)(bi * stride) * nx + bj * stride;
    int nan = 0, cnt = 0;
    for (int pix = lane; pix < nd * nd; pix += 64) {
      const float v = p[(long)(pix / nd) * nx + pix % nd];
      nan |= v != v;
      cnt += v > thresh;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      nan |= __shfl_down(nan, off, 64);
      cnt += __shfl_down(cnt, off, 64);
    }
    if (lane == 0) valid[b] = (!nan && cnt >= n_thresh) ? 1 : 0;
  }
}
