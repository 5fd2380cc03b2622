// What the evaluations of an hourly array (..., 24, ny, nx) share on the host: the plain constants (rdgan_hourly.hip.h adds the
// device helpers on top of them), and what the accumulate entries (rdgan_eval_entries.h: temporal, cells, storms, areal, catchment,
// space-time, cascade) check and size the same way: the layout of the array, the 16-byte route, the levels in units, the units of a
// pass; and how the joint-field scores and the rank histograms admit an ensemble against observed days.  Host-only and free of HIP: a plain C++ compiler builds this header on its own (tests/test_hourly_host.py does).
#pragma once
#include <math.h>

#define RD_HOURS 24                         // hours of a day: the third axis from the right of every hourly array
#define RD_HOURLY_MAXPLANE (1L << 24)       // pixels of a plane
#define RD_HOURLY_MAXELEMS (1L << 40)       // elements of one call's array
// depths in fixed point: q = rint(x * RD_DEPTH_UNIT) in fp32, ties to even, for an hourly value 0 <= x < RD_DEPTH_MAX
#define RD_DEPTH_UNIT 1024
#define RD_DEPTH_MAX 2048

// true when none of the pointers has a bit of `mask` set: rd_aligned(7, counts, workspace), a null pointer passes
template <typename... P>
static bool rd_aligned(unsigned long long mask, P... p) {
  return !((... | (unsigned long long)p) & mask);
}

// n >= 1 days, day d at x + d * day_stride: the stride no less than a day, and n * day_stride at most 2^50 elements
static bool rd_day_stride_ok(long n, long day_stride, long day_elems) {
  return n >= 1 && day_stride >= day_elems && day_stride <= (1L << 50) / n;
}

// the array an accumulate entry reads: x on 4 bytes, 1 <= n days of day_elems >= 1 elements each, at most RD_HOURLY_MAXELEMS in all
static bool rd_hourly_layout_ok(const void* x, long n, long day_stride, long day_elems) {
  return rd_aligned(3, x) && day_elems >= 1 && n >= 1 && n <= RD_HOURLY_MAXELEMS / day_elems && rd_day_stride_ok(n, day_stride, day_elems);
}

// an ensemble of 1 <= m <= max_m members against 1 <= n_days <= max_days observed days of 24 ny nx values, shared by the days or one
// per day: the call's members, and m + extra vectors (the ranks count the observation in: 1), within RD_HOURLY_MAXELEMS
static bool rd_ensemble_shape_ok(long m, long n_days, long ny, long nx, int shared, long max_m, long max_days, long extra) {
  if (m < 1 || m > max_m || n_days < 1 || n_days > max_days || (shared != 0 && shared != 1)) return false;
  if (ny < 1 || nx < 1 || ny > RD_HOURLY_MAXPLANE || nx > RD_HOURLY_MAXPLANE || ny * nx > RD_HOURLY_MAXPLANE) return false;
  const long held = RD_HOURLY_MAXELEMS / (RD_HOURS * ny * nx);
  return m + extra <= held && (shared ? 1 : n_days) * m <= held;
}

// 16-byte loads of four adjacent values (rd_load<4>): every row of every day starts on 16 bytes, rows being `row` elements apart
// (a plane, or nx) and days day_stride
static bool rd_vec4_ok(const void* x, long row, long day_stride) {
  return rd_aligned(15, x) && row % 4 == 0 && day_stride % 4 == 0;
}

// 0 <= L <= maxL levels of a day's depth, each in 0 .. RD_DEPTH_MAX * RD_HOURS and strictly increasing -> out[i] in units
static bool rd_levels_q(const double* levels, int L, int maxL, long long* out) {
  if (L < 0 || L > maxL || (L > 0 && !levels)) return false;
  for (int i = 0; i < L; ++i) {
    if (!(levels[i] >= 0.0 && levels[i] <= (double)RD_DEPTH_MAX * RD_HOURS) || (i > 0 && !(levels[i] > levels[i - 1]))) return false;
    out[i] = llrint(levels[i] * (double)RD_DEPTH_UNIT);
  }
  return true;
}

// the units (planes or days) of a pass: as many as workspace_bytes hold, at most n_units and max_units; 0 when it holds none (a
// negative size counts as 0), which an entry refuses
static long rd_pass_units(long workspace_bytes, long unit_bytes, long n_units, long max_units) {
  long held = workspace_bytes < 0 ? 0 : workspace_bytes / unit_bytes;
  if (held > n_units) held = n_units;
  return held > max_units ? max_units : held;
}
