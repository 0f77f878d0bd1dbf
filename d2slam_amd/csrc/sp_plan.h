// sp_plan.h -- the SuperPoint network as data, stated once: its layers in order and the sizes of their outputs (floored, as a call computes them, and as a
// handle allocates them), the layout of exact_order's crop batch, and the packings the weights are uploaded in.  superpoint_host.hip checks, packs, allocates,
// launches and reads back from these tables.  Plain C++ (no HIP): tests/cpp/sp_plan_test.cpp exercises it on the host.
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

// floats per image a handle ALLOCATES for a layer's output at its maximum size: not the floored size, so that no buffer is smaller than the area suggests where
// the maximum is no multiple of 8.  SP_PA stands for the buffer the heads share (convPa alone, or convPa | convDa)
constexpr size_t sp_alloc_floats(int layer, size_t Hmax, size_t Wmax) {
  return Hmax * Wmax * (layer == SP_PA ? SP_PADA_COUT : SP_PLAN[layer].cout) >> (2 * sp_out_level(layer));
}

// exact_order's crop batch (E x E crops through conv1b .. convPb, then a dense E x E score map), stored tensor by tensor: the output of `layer` for a batch of
// C crops begins C * sp_crop_off(layer, E) floats into the buffer, the score maps at layer = SP_PB + 1, and a crop takes sp_crop_floats(E) in all
constexpr size_t sp_crop_off(int layer, int E) { size_t o = 0; for (int i = SP_1B; i < layer; ++i) o += sp_out_floats(i, E, E); return o; }
constexpr size_t sp_crop_floats(int E) { return sp_crop_off(SP_PB + 1, E) + (size_t)E * E; }

// the packings d2fe_load_superpoint uploads (Layer records of SpNet::L), in upload order
enum { L_1B = 0, L_2A, L_2B, L_3A, L_3B, L_4A, L_4B, L_PADA, L_PB, L_DB, L_PA, L_DA32, L_DB32,      // the last three: sparse descriptor head
       L_X1B, L_X2A, L_X2B, L_X3A, L_X3B, L_X4A, L_X4B, L_XPA,     // exact_order: direct fp32 packings of the eight Winograd layers of the detector path
       L_COUNT };
enum { SP_ALWAYS = 0, SP_WITH_SPARSE, SP_WITH_EXACT };      // a packing exists: on every handle / with the sparse descriptor head / with exact_order
// part[0 .. nparts): the plan layers it concatenates along the output channels (they share their input); f32: exact fp32 fragments whatever the handle's precision
struct SpPack { int nparts, part[2], cout_pad; bool f32; int when; };
constexpr SpPack SP_PACK[L_COUNT] = {
    {1, {SP_1B, 0}, 64, false, SP_ALWAYS},
    {1, {SP_2A, 0}, 64, false, SP_ALWAYS},
    {1, {SP_2B, 0}, 64, false, SP_ALWAYS},
    {1, {SP_3A, 0}, 128, false, SP_ALWAYS},
    {1, {SP_3B, 0}, 128, false, SP_ALWAYS},
    {1, {SP_4A, 0}, 128, false, SP_ALWAYS},
    {1, {SP_4B, 0}, 128, false, SP_ALWAYS},
    {2, {SP_PA, SP_DA}, 512, false, SP_ALWAYS},      // L_PADA: convPa | convDa share their input
    {1, {SP_PB, 0}, 128, false, SP_ALWAYS},
    {1, {SP_DB, 0}, 256, false, SP_ALWAYS},
    {1, {SP_PA, 0}, 256, false, SP_WITH_SPARSE},     // the detector head alone in the mode's precision; the descriptor head always as exact fp32 fragments
    {1, {SP_DA, 0}, 256, true, SP_WITH_SPARSE},
    {1, {SP_DB, 0}, 256, true, SP_WITH_SPARSE},
    {1, {SP_1B, 0}, 64, true, SP_WITH_EXACT},        // the detector path once more as direct fp32 fragments (convPb is direct in every fp32 mode)
    {1, {SP_2A, 0}, 64, true, SP_WITH_EXACT},
    {1, {SP_2B, 0}, 64, true, SP_WITH_EXACT},
    {1, {SP_3A, 0}, 128, true, SP_WITH_EXACT},
    {1, {SP_3B, 0}, 128, true, SP_WITH_EXACT},
    {1, {SP_4A, 0}, 128, true, SP_WITH_EXACT},
    {1, {SP_4B, 0}, 128, true, SP_WITH_EXACT},
    {1, {SP_PA, 0}, 256, true, SP_WITH_EXACT},
};
// the chain launcher walks a packing set by plan layer
static_assert(L_4B - L_1B == SP_4B - SP_1B && L_XPA - L_X1B == SP_PA - SP_1B, "the chain's packings are in plan order");

}  // namespace d2fe
