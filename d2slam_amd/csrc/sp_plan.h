// sp_plan.h -- the SuperPoint network as data: its layers, in order, and the floored sizes of their outputs.  d2fe_debug_read (api.hip) sizes the tensors
// it hands out from this table.  Plain C++ (no HIP): tests/cpp/sp_plan_test.cpp exercises it on the host.
#pragma once
#include <stddef.h>

#include "../../include/d2fe.h"

namespace d2fe {

// the layers in the order of d2fe_superpoint_weights::layer; SP_1B .. SP_PB is the detector path, a chain: every layer reads its predecessor's output
enum { SP_1A = 0, SP_1B, SP_2A, SP_2B, SP_3A, SP_3B, SP_4A, SP_4B, SP_PA, SP_PB, SP_DA, SP_DB, SP_NLAYERS };
static_assert(SP_NLAYERS == D2FE_SP_NUM_LAYERS, "the plan follows the weight container");

struct SpLayer {
  const char* name;      // d2fe_debug_read / weight container name
  int cin, cout, ks;
  int level;             // pool level of the input: the layer runs at (H >> level) x (W >> level)
  bool pool;             // a 2x2 max-pool (floors) behind the convolution
};

constexpr SpLayer SP_PLAN[SP_NLAYERS] = {
    {"conv1a", 1, 64, 3, 0, false},
    {"conv1b", 64, 64, 3, 0, true},
    {"conv2a", 64, 64, 3, 1, false},
    {"conv2b", 64, 64, 3, 1, true},
    {"conv3a", 64, 128, 3, 2, false},
    {"conv3b", 128, 128, 3, 2, true},
    {"conv4a", 128, 128, 3, 3, false},
    {"conv4b", 128, 128, 3, 3, false},
    {"convPa", 128, 256, 3, 3, false},
    {"convPb", 256, 65, 1, 3, false},
    {"convDa", 128, 256, 3, 3, false},
    {"convDb", 256, 256, 1, 3, false},
};
constexpr int SP_CELL_LEVEL = 3;      // the heads run on the 8x8 cells
constexpr int SP_PADA_COUT = SP_PLAN[SP_PA].cout + SP_PLAN[SP_DA].cout;      // the dense head's convPa | convDa share one buffer

// floats per image of a `ch`-channel NHWC tensor at pool level `level` of an H x W image: the pools floor
constexpr size_t sp_floats(int level, int ch, int H, int W) { return (size_t)(H >> level) * (size_t)(W >> level) * ch; }
constexpr int sp_out_level(int layer) { return SP_PLAN[layer].level + (SP_PLAN[layer].pool ? 1 : 0); }
constexpr int sp_out_h(int layer, int H) { return H >> sp_out_level(layer); }
constexpr int sp_out_w(int layer, int W) { return W >> sp_out_level(layer); }
constexpr size_t sp_out_floats(int layer, int H, int W) { return sp_floats(sp_out_level(layer), SP_PLAN[layer].cout, H, W); }

}  // namespace d2fe
