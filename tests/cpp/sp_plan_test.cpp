// The SuperPoint layer plan (d2slam_amd/csrc/sp_plan.h) on the host: prints, for each H x W given on the command line, every layer's shape and its output
// height, width, channels and floats per image, the size of the dense head's convPa | convDa tensor and the floats per image a handle of that maximum size
// allocates per activation buffer; then the layout of exact_order's 88 x 88 crop batch and the packing table.  tests/test_sp_plan_cpu.py compares the lines
// with its own arithmetic.
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
    for (int i = SP_1A; i <= SP_PA; ++i) printf("alloc %d %d %s %zu\n", H, W, SP_PLAN[i].name, sp_alloc_floats(i, H, W));
  }
  for (int i = SP_1B; i <= SP_PB; ++i) printf("crop %s %zu\n", SP_PLAN[i].name, sp_crop_off(i, 88));
  printf("crop scores %zu\ncrop total %zu\n", sp_crop_off(SP_PB + 1, 88), sp_crop_floats(88));
  for (int i = 0; i < L_COUNT; ++i) {
    const SpPack& k = SP_PACK[i];
    printf("pack %d %s %s %d %d %d\n", i, SP_PLAN[k.part[0]].name, k.nparts == 2 ? SP_PLAN[k.part[1]].name : "-", k.cout_pad, (int)k.f32, k.when);
  }
  return 0;
}
