// csrc/rdgan_options.h compiled WITHOUT HIP (tests/test_options_host.py): one line per RD_OPTIONS row --
//   name  alias|-  table default  default-constructed RdOptions field  forms mask  rd_option_normalise at each probe value (x = refused)
// and one line with rd_form_key of the defaults for each network.
#include <stdio.h>
#include "../../pr_disagg_radar_gan_amd/csrc/rdgan_options.h"

int main() {
  static const int probes[] = {-5, -1, 0, 1, 2, 3, 9, 100};
  const RdOptions defaults;
  for (const RdOptionRow& r : RD_OPTIONS) {
    printf("%s %s %d %d %u", r.name, r.alias ? r.alias : "-", r.def, defaults.*r.field, r.forms);
    for (int p : probes) {
      int v = 12345;
      if (rd_option_normalise(r, p, &v)) printf(" %d", v);
      else printf(" %s", v == 12345 && r.refusal ? "x" : "?");      // a refusal leaves *out alone and has a message
    }
    printf("\n");
  }
  printf("keys %d %d\n", rd_form_key(&defaults, RD_FORMS_GEN), rd_form_key(&defaults, RD_FORMS_CRITIC));
  // a form key tells two states of any one flagged option apart
  int clashes = 0;
  for (const RdOptionRow& r : RD_OPTIONS)
    for (unsigned forms = RD_FORMS_GEN; forms <= RD_FORMS_CRITIC; forms <<= 1) {
      if (!(r.forms & forms)) continue;
      for (int a = r.lo; a <= r.hi; ++a)
        for (int b = a + 1; b <= r.hi; ++b) {
          RdOptions x, y;
          x.*r.field = a; y.*r.field = b;
          if (rd_form_key(&x, forms) == rd_form_key(&y, forms) || rd_form_key(&x, forms) < 0) { printf("clash %s %d %d\n", r.name, a, b); ++clashes; }
        }
    }
  printf("clashes %d\n", clashes);
  return clashes ? 1 : 0;
}
