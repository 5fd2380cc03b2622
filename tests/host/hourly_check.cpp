// csrc/rdgan_hourly_host.h compiled WITHOUT HIP and with the address and undefined-behaviour sanitizers
// (tests/test_hourly_host.py): one line "name value" per probe of rd_hourly_layout_ok, rd_pass_units, rd_aligned and rd_vec4_ok at
// their edges; the test holds the expected values.
#include <stdio.h>
#include "../../pr_disagg_radar_gan_amd/csrc/rdgan_hourly_host.h"

int main() {
  alignas(16) static float buf[8];
  const void* x = buf;
  const void* odd = (const char*)buf + 2;
  const long day = 24 * 35, cap = 1L << 40, span = 1L << 50;
  // the layout: n, the stride against the day, n * day_stride against 2^50, n * day_elems against 2^40, the alignment of x
  printf("layout_good %d\n", rd_hourly_layout_ok(x, 3, day, day));
  printf("layout_n0 %d\n", rd_hourly_layout_ok(x, 0, day, day));
  printf("layout_n_negative %d\n", rd_hourly_layout_ok(x, -1, day, day));
  printf("layout_day0 %d\n", rd_hourly_layout_ok(x, 3, day, 0));
  printf("layout_stride_below_day %d\n", rd_hourly_layout_ok(x, 3, day - 1, day));
  printf("layout_stride_is_day %d\n", rd_hourly_layout_ok(x, 3, day, day));
  printf("layout_stride_at_span %d\n", rd_hourly_layout_ok(x, 3, span / 3, day));
  printf("layout_stride_above_span %d\n", rd_hourly_layout_ok(x, 3, span / 3 + 1, day));
  printf("layout_one_day_any_stride %d\n", rd_hourly_layout_ok(x, 1, span, day));
  printf("layout_one_day_above_span %d\n", rd_hourly_layout_ok(x, 1, span + 1, day));
  printf("layout_elems_at_cap %d\n", rd_hourly_layout_ok(x, cap / 1024, 1024, 1024));
  printf("layout_elems_one_day_over %d\n", rd_hourly_layout_ok(x, cap / 1024 + 1, 1024, 1024));
  printf("layout_one_day_of_cap %d\n", rd_hourly_layout_ok(x, 1, cap, cap));
  printf("layout_one_day_over_cap %d\n", rd_hourly_layout_ok(x, 1, cap + 1, cap + 1));
  printf("layout_x_misaligned %d\n", rd_hourly_layout_ok(odd, 3, day, day));
  printf("layout_x_on_4 %d\n", rd_hourly_layout_ok((const char*)buf + 4, 3, day, day));
  // the pass: what the workspace holds, capped by the input and by the entry's limit
  const long unit = 35 * 16 + 8;
  printf("pass_negative %ld\n", rd_pass_units(-5, unit, 72, 65535));
  printf("pass_zero %ld\n", rd_pass_units(0, unit, 72, 65535));
  printf("pass_below_unit %ld\n", rd_pass_units(unit - 1, unit, 72, 65535));
  printf("pass_one_unit %ld\n", rd_pass_units(unit, unit, 72, 65535));
  printf("pass_below_two %ld\n", rd_pass_units(2 * unit - 1, unit, 72, 65535));
  printf("pass_five %ld\n", rd_pass_units(5 * unit, unit, 72, 65535));
  printf("pass_more_than_input %ld\n", rd_pass_units(100 * unit, unit, 72, 65535));
  printf("pass_more_than_max %ld\n", rd_pass_units(70000 * unit, unit, 1L << 20, 65535));
  printf("pass_at_max %ld\n", rd_pass_units(65535 * unit, unit, 1L << 20, 65535));
  printf("pass_largest_size %ld\n", rd_pass_units(0x7FFFFFFFFFFFFFFFL, 1, 1L << 40, 2730));
  // alignment of several pointers at once; a null pointer passes
  printf("aligned_all %d\n", rd_aligned(7, (const void*)buf, (const void*)(buf + 2), (const void*)nullptr));
  printf("aligned_one_on_4 %d\n", rd_aligned(7, (const void*)buf, (const void*)(buf + 1)));
  printf("aligned_4_is_enough %d\n", rd_aligned(3, (const void*)(buf + 1)));
  // the 16-byte route: the pointer on 16 bytes, the row and the day stride multiples of 4
  printf("vec4_aligned %d\n", rd_vec4_ok(x, 4 * 8, 24 * 32 + 4));
  printf("vec4_off_by_4_bytes %d\n", rd_vec4_ok((const char*)buf + 4, 4 * 8, 24 * 32 + 4));
  printf("vec4_plane_not_of_4 %d\n", rd_vec4_ok(x, 5 * 7, 24 * 35));
  printf("vec4_stride_not_of_4 %d\n", rd_vec4_ok(x, 4 * 8, 24 * 32 + 2));
  return 0;
}
