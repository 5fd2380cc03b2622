// What the accumulate entries of the hourly evaluations (rdgan_eval_entries.h: temporal, cells, storms, areal, space-time) check
// and size the same way: the layout of the hourly array and the units of a pass.  Host-only and free of HIP: a plain C++ compiler
// builds this header on its own (tests/test_hourly_host.py does).
#pragma once

#define RD_HOURLY_MAXELEMS (1L << 40)       // elements of one call's array; every RD_*_MAXELEMS of the device headers equals it

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

// the units (planes or days) of a pass: as many as workspace_bytes hold, at most n_units and max_units; 0 when it holds none (a
// negative size counts as 0), which an entry refuses
static long rd_pass_units(long workspace_bytes, long unit_bytes, long n_units, long max_units) {
  long held = workspace_bytes < 0 ? 0 : workspace_bytes / unit_bytes;
  if (held > n_units) held = n_units;
  return held > max_units ? max_units : held;
}
