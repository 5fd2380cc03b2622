// csrc/rdgan_hourly_host.h compiled WITHOUT HIP and with the address and undefined-behaviour sanitizers
// (tests/test_hourly_host.py): one line "name value" per probe of rd_hourly_layout_ok, rd_pass_units, rd_aligned, rd_vec4_ok and
// rd_ensemble_shape_ok at their edges; the test holds the expected values.
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
  // an ensemble against observed days: the scores (8192 members, no extra vector) and the ranks (4095, the observation as one more),
  // 2^20 days either; a plane of 4096 x 4096 leaves room for 2730 vectors of 24 planes
  const long days = 1L << 20;
  auto scores = [&](long m, long D, long ny, long nx, int shared) { return (int)rd_ensemble_shape_ok(m, D, ny, nx, shared, 8192, days, 0); };
  auto ranks = [&](long m, long D, long ny, long nx, int shared) { return (int)rd_ensemble_shape_ok(m, D, ny, nx, shared, 4095, days, 1); };
  printf("ens_scores_good %d\n", scores(5, 2, 3, 5, 0));
  printf("ens_scores_most %d\n", scores(8192, days, 1, 1, 0));
  printf("ens_scores_m0 %d\n", scores(0, 2, 3, 5, 0));
  printf("ens_scores_m_over %d\n", scores(8193, 2, 3, 5, 0));
  printf("ens_scores_days0 %d\n", scores(5, 0, 3, 5, 0));
  printf("ens_scores_days_over %d\n", scores(5, days + 1, 3, 5, 0));
  printf("ens_scores_ny0 %d\n", scores(5, 2, 0, 5, 0));
  printf("ens_scores_nx0 %d\n", scores(5, 2, 3, 0, 0));
  printf("ens_scores_plane_over %d\n", scores(5, 2, 4097, 4097, 0));
  printf("ens_scores_side_over %d\n", scores(5, 2, (1L << 24) + 1, 1, 0));
  printf("ens_scores_shared2 %d\n", scores(5, 2, 3, 5, 2));
  printf("ens_scores_shared_negative %d\n", scores(5, 2, 3, 5, -1));
  printf("ens_scores_fill_the_cap %d\n", scores(2730, 1, 4096, 4096, 0));
  printf("ens_scores_one_over_the_cap %d\n", scores(2731, 1, 4096, 4096, 0));
  printf("ens_ranks_good %d\n", ranks(5, 2, 3, 5, 0));
  printf("ens_ranks_most %d\n", ranks(4095, days, 1, 1, 1));
  printf("ens_ranks_m0 %d\n", ranks(0, 2, 3, 5, 0));
  printf("ens_ranks_m_over %d\n", ranks(4096, 2, 3, 5, 0));
  printf("ens_ranks_days0 %d\n", ranks(5, 0, 3, 5, 0));
  printf("ens_ranks_days_over %d\n", ranks(5, days + 1, 3, 5, 0));
  printf("ens_ranks_ny0 %d\n", ranks(5, 2, 0, 5, 0));
  printf("ens_ranks_nx0 %d\n", ranks(5, 2, 3, 0, 0));
  printf("ens_ranks_plane_over %d\n", ranks(5, 2, 4097, 4097, 0));
  printf("ens_ranks_shared2 %d\n", ranks(5, 2, 3, 5, 2));
  printf("ens_ranks_shared_negative %d\n", ranks(5, 2, 3, 5, -1));
  printf("ens_ranks_vectors_over_the_cap %d\n", ranks(4095, 2, 4096, 4096, 0));
  printf("ens_ranks_observation_fits %d\n", ranks(2729, 1, 4096, 4096, 0));
  printf("ens_ranks_observation_is_one_too_many %d\n", ranks(2730, 1, 4096, 4096, 0));
  printf("ens_ranks_per_day_members_over_the_cap %d\n", ranks(2048, days, 64, 64, 0));
  printf("ens_ranks_shared_members_fit %d\n", ranks(2048, days, 64, 64, 1));
  return 0;
}
