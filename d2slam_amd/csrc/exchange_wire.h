// exchange_wire.h -- what the stereo exchange (exchange.hip, which defines all of it) and the quad exchange (quad_exchange.hip) share:
//   the ONE dlopen table of librccl: the library is loaded once per process, at run time, only when a communicator is made or used;
//   the wire half of an exchange: the per-slot block buffers, the shared part of the configuration, the stream choice and the round
//   pack_blocks(_int8) -> ONE all-gather (RCCL or the caller's collective) -> [int8: decode].
// What an exchange does with the gathered blocks (counts, gate, the matcher's problem table) stays in its own file.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "consumer.h"

namespace d2fe {

// the five RCCL entry points the exchanges need; ncclComm_t and ncclUniqueId stay opaque (a pointer; 128 bytes)
struct Rccl {
  struct Uid { char b[128]; };       // ncclUniqueId: 128 bytes, passed BY VALUE to ncclCommInitRank
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Uid, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::string path;
};
extern Rccl g_rccl;
int rccl_load(const char* path);             // D2FE_OK, or D2FE_ERR_UNSUPPORTED when no librccl can be loaded; idempotent
int rccl_fail(const char* what, int rc);     // records "<what>: <ncclGetErrorString>" and returns D2FE_ERR_HIP

// a result slot with the blocks of one round: this rank's packed blocks and everybody's gathered ones, fp32 and (int8 wire forms only) as they travel
struct WireSlot : SlotBase {
  float* d_blocks = nullptr; int8_t* d_blocks_q = nullptr; float* d_gath = nullptr; int8_t* d_gath_q = nullptr;
};

// the wire half of an exchange object; d2fe_exchange_s and d2fe_quad_exchange_s derive from it
struct Wire {
  PipeRef pipe;
  d2fe_handle h = nullptr;
  void* comm = nullptr;                                                    // ncclComm_t, or null: the callback
  d2fe_all_gather_fn all_gather = nullptr; void* all_gather_user = nullptr;
  int world = 1, wire = D2FE_WIRE_FP32;
  int NB = 0, cap = 0, D = 256, G = 0;                                     // blocks this rank sends per round (stereo: frames; quad: 4 * quads), their geometry (D: floats per descriptor row)
  int rows = 0;                                                            // descriptor rows (of D floats) one fp32 block spans: the matcher's offsets count them
  int BLK = 0, BLKB = 0, n_off = 0, g_off = 0;                             // words of an fp32 block, bytes of an int8 one, the count and NetVLAD fields of an fp32 block
  bool int8 = false;
  hipStream_t own = nullptr;       // cfg.own_stream: the one stream of its own (round 5's placement), else the lanes' streams
};

// the configuration fields the two exchanges share; `own_bad`: what the caller found wrong with its own fields; noun: "exchange" / "quad exchange"
template <class Cfg>
int wire_check_config(const Cfg& cfg, bool own_bad, const void* nccl_comm, const char* noun) {
  if (cfg.world < 1 || cfg.rank < 0 || cfg.rank >= cfg.world || cfg.slots < 1 || cfg.slots > 64 || cfg.wire < 0 || cfg.wire > 2 || own_bad)
    return ctx_fail(D2FE_ERR_INVALID, std::string("bad ") + noun + " configuration");
  if (cfg.world == 1 && !cfg.loopback) return ctx_fail(D2FE_ERR_INVALID, "one rank and no loopback: nothing to exchange");
  if (!nccl_comm && !cfg.all_gather) return ctx_fail(D2FE_ERR_INVALID, "neither an RCCL communicator nor an all-gather callback");
  return D2FE_OK;
}
// the geometry of the blocks of a pipe with n_blocks rows of `cap` keypoints of D floats and a G-float NetVLAD descriptor per round
template <class Cfg>
int wire_init(Wire& w, PipeRef pipe, void* nccl_comm, const Cfg& cfg, int n_blocks, int cap, int D, int G) {
  w.pipe = pipe; w.h = pipe.handle(); w.comm = nccl_comm; w.all_gather = cfg.all_gather; w.all_gather_user = cfg.all_gather_user;
  w.world = cfg.world; w.wire = cfg.wire; w.int8 = cfg.wire != D2FE_WIRE_FP32;
  w.NB = n_blocks; w.cap = cap; w.D = D; w.G = G;
  w.BLK = d2fe_block_words_d(cap, D, G); w.BLKB = d2fe_block_bytes_int8_d(cap, D, G);
  if (w.BLK < 0 || w.BLKB < 0) return D2FE_ERR_INVALID;      // d2fe_block_words_d has said why
  // the matcher addresses the b side in place, in rows of D floats from the start of the gathered buffer: every block must start on a row (256 % D == 0: D = 4 .. 256
  // in powers of two, 64 among them; any other width that happens to divide the block)
  if (w.BLK % D) return ctx_fail(D2FE_ERR_UNSUPPORTED, "blocks of " + std::to_string(w.BLK) + " words do not start on a descriptor row of " + std::to_string(D) + " floats: the matcher cannot read them in place");
  w.rows = w.BLK / D;
  if (w.int8 && (cap * D + G + cap * 8) % 4) return ctx_fail(D2FE_ERR_UNSUPPORTED, "int8 blocks of this capacity / descriptor width / NetVLAD size do not keep their count word aligned");
  w.n_off = d2fe_block_field_offset_d(cap, D, G, 4); w.g_off = d2fe_block_field_offset_d(cap, D, G, 3);
  return D2FE_OK;
}
int wire_alloc_blocks(const Wire& w, WireSlot& S);      // the blocks of one slot, zeroed
void wire_free_slot(WireSlot& S);                       // waits for the slot's round, then frees the blocks and the slot
void wire_destroy_stream(Wire& w);
int wire_gathered(const Wire& w, const WireSlot& S, const float** d_blocks, const void** d_wire_blocks);
int wire_stream(const Wire& w, int64_t ticket, hipStream_t* st);      // the exchange's own stream, or the stream of the lane that produced the ticket
// pack the view's NB rows -> mark 1 -> ONE all-gather -> mark 2 -> [int8: decode into S.d_gath]; the caller has recorded mark 0
int wire_round(const Wire& w, WireSlot& S, const TicketView& v, hipStream_t st);

}  // namespace d2fe
