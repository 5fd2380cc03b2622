// The vocabulary the kernels of the hourly evaluations share (verification, temporal, cells, storms, areal, catchments, space-time,
// analogs, joint scores, cascade): the constants of rdgan_hourly_host.h, the two definitions of a bad value, the fixed-point depth,
// the 1-or-4-wide load, and the thresholds.  Nothing else lives here.  Every helper is inlined
// into its caller.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hostplan.h"              // RDGAN_NHOURS
#include "rdgan_hourly_host.h"           // RD_HOURS, RD_HOURLY_MAXPLANE, RD_HOURLY_MAXELEMS, RD_DEPTH_UNIT, RD_DEPTH_MAX

static_assert(RD_HOURS == RDGAN_NHOURS, "the evaluations read the hourly arrays the network writes");

#define RD_THR_MAX 8                     // thresholds of one call
#define RD_F32_EXP 0x7F800000u           // the exponent bits of an fp32: all set in a NaN and in +-inf

// the thresholds as the kernels compare them (rd_thresholds): fp32, >= 0, strictly increasing
struct rd_thr {
  float v[RD_THR_MAX];
};

// Two definitions of a bad value, and an evaluation uses one of them.  Non-finite: NaN or +-inf (temporal, cells, storms,
// space-time, which compare fp32 values with thresholds).  Out of the depth range: NaN, +-inf, negative or >= RD_DEPTH_MAX (areal,
// catchments, analogs, cascade, which add depths in fixed point).
__device__ __forceinline__ bool rd_nonfinite(float v) { return (__float_as_uint(v) & RD_F32_EXP) == RD_F32_EXP; }
__device__ __forceinline__ bool rd_depth_bad(float v) { return !(v >= 0.0f && v < (float)RD_DEPTH_MAX); }
// the depth in units of 1 / RD_DEPTH_UNIT: the fp32 product rounded to the nearest integer, ties to even; below 2^21 for a good v
__device__ __forceinline__ int rd_depth_q(float v) { return (int)rintf(v * (float)RD_DEPTH_UNIT); }

// V = 4: one 16-byte load, p on 16 bytes (rd_vec4_ok); V = 1: a scalar load
template <int V> __device__ __forceinline__ void rd_load(const float* p, float (&v)[V]) {
  static_assert(V == 1 || V == 4, "one value or four");
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}
