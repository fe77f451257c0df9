// Host entries of the copy-engine allreduce's kernels (sdma_comm.hip) and their launch
// arguments; SdmaComm (sdma_comm.cc, host C++) fills SdmaLaunch and calls them.
#pragma once

#include <hip/hip_runtime_api.h>

#include "../runtime/sdma_schedule.h"
#include "xgmi_comm.h"

namespace mxar {

// One launch of the pipelined reduce / gather for the local ranks of a call (blockIdx.y).
struct SdmaRankArgs {
  const char* in;         // the rank's input (whole tensor segment)
  char* out;              // its output
  const char* sd;         // its SD slots of this call's parity (slot s at s * slot)
  const char* rd;         // its RD slots of this call's parity
  const uint32_t* flags;  // its flag words (sdma_fs_word / sdma_fr_word)
  int64_t* mid[kSdmaMaxPieces];  // phase-2 release signal of each piece (value pointer)
  uint32_t* cnt;          // per-piece workgroup tickets (device, zero between launches)
  uint32_t* err;
  uint32_t epoch;
  int r;
};
struct SdmaLaunch {
  SdmaRankArgs y[kSdmaMaxLocal];
  int64_t n, block, pe, slot;  // elements (slot: bytes)
  uint64_t timeout;            // 100 MHz ticks
  int W, K;
  float scale;
};

// One lane stores 0 to the signal value at `sig` (system scope): the call's copies start.
void launch_sdma_release(int64_t* sig, hipStream_t s);
// The pipelined reduce, then (W > 1) the pipelined gather: dim3(grid, ny) each.
void launch_sdma_reduce_gather(const SdmaLaunch& L, int grid, int ny, hipStream_t s, DType dt);

}  // namespace mxar
