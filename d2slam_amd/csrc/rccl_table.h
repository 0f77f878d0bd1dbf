// rccl_table.h -- the ONE dlopen table of librccl that the stereo exchange (exchange.hip, which defines it) and the quad exchange (quad_exchange.hip) share:
// the library is loaded once per process, at run time, only when a communicator is made or used.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

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

}  // namespace d2fe
