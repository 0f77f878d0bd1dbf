// The SuperPoint layer plan (d2slam_amd/csrc/sp_plan.h) on the host: prints, for each H x W given on the command line, every layer's shape and its output
// height, width, channels and floats per image, and the size of the dense head's convPa | convDa tensor.  tests/test_sp_plan_cpu.py compares the lines with
// its own arithmetic.
#include <cstdio>
#include <cstdlib>

#include "sp_plan.h"

using namespace d2fe;

int main(int argc, char** argv) {
  for (int a = 1; a + 1 < argc; a += 2) {
    const int H = atoi(argv[a]), W = atoi(argv[a + 1]);
    for (int i = 0; i < SP_NLAYERS; ++i)
      printf("layer %d %d %s %d %d %d %zu shape %d %d %d\n", H, W, SP_PLAN[i].name, sp_out_h(i, H), sp_out_w(i, W), SP_PLAN[i].cout, sp_out_floats(i, H, W),
             SP_PLAN[i].cout, SP_PLAN[i].cin, SP_PLAN[i].ks);
    printf("head %d %d convPaDa %d %zu\n", H, W, SP_PADA_COUT, sp_floats(SP_CELL_LEVEL, SP_PADA_COUT, H, W));
  }
  return 0;
}
