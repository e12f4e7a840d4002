// Stand-alone host program over pinot_amd/csrc/civil.h (tests/test_time_transform.py builds it with
// -fsanitize=address,undefined and runs it as it is): reads lines "function unit in_mul in_div out_mul out_div value"
// and prints per line the program's validity, whether the value fits, and the transformed value.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../pinot_amd/csrc/civil.h"

int main() {
  phip::TimeProgram p;
  int64_t v;
  std::vector<int64_t> out;
  while (scanf("%d %d %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &p.function, &p.unit, &p.in_mul, &p.in_div,
               &p.out_mul, &p.out_div, &v) == 7) {
    const bool valid = phip::time_program_valid(p);
    const bool fits = valid && phip::time_transform_fits(p, v, v);
    printf("%d %d %" PRId64 "\n", valid ? 1 : 0, fits ? 1 : 0, fits ? phip::time_transform(p, v) : 0);
  }
  return 0;
}
