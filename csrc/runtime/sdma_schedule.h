// The copy-engine allreduce (SdmaComm, csrc/hip/sdma_comm.cc) as pure functions of the
// communicator's knobs and the call's shape: no HIP, no HSA, no environment. The slab map and
// the block length are constexpr, so the kernels (sdma_comm.hip) and the host read the same
// ones. SdmaComm::plan waits for its signal slot, asks plan_sdma_copies for the segment's
// schedule, arms the signals to the schedule's counts and submits the list in order;
// tests/test_sdma_schedule.py pins every rule against a table recorded from the code before
// the split, csrc/tests/runtime_stress.cc checks what the engines and kernels rely on.
#pragma once

#include <cstdint>
#include <vector>

namespace mxar {

constexpr int kSdmaMaxPieces = 8;  // pipeline pieces per block at most
constexpr int kSdmaMaxLocal = 8;   // local ranks one reduce / gather launch serves
constexpr int kSdmaSlots = 16;     // calls in flight at most (signal / epoch-word ring)
constexpr int kSdmaMaxWorld = 32;
constexpr int64_t kFlagBytes = 64 * 1024;
constexpr int kFrWord = kSdmaMaxWorld * kSdmaMaxPieces;
constexpr int64_t kPieceBytes = int64_t{64} << 20;  // auto pieces: one per 64 MiB of the block (2..8)

// The slab of a rank: [flag words | SD[2][W] slots | RD[2][W] slots]. FS[s][k] (u32 words):
// rank s's piece k of the own block has arrived in SD[par][s]; FR[s][k]: rank s's reduced
// piece k has arrived in RD[par][s] (s = the own rank: the engines have read the own piece).
// `par` is the call epoch's parity: a rank is at most one call ahead of a peer still reading.
constexpr int64_t sdma_fs_word(int s, int k) { return int64_t{s} * kSdmaMaxPieces + k; }
constexpr int64_t sdma_fr_word(int s, int k) { return kFrWord + int64_t{s} * kSdmaMaxPieces + k; }
constexpr int64_t sdma_sd_off(int W, int64_t slot, int par, int src) {
  return kFlagBytes + (static_cast<int64_t>(par) * W + src) * slot;
}
constexpr int64_t sdma_rd_off(int W, int64_t slot, int par, int src) {
  return kFlagBytes + ((2 + static_cast<int64_t>(par)) * W + src) * slot;
}
// Elements of block s of a segment of n elements in blocks of `block`.
constexpr int64_t sdma_block_len(int64_t n, int64_t block, int s) {
  const int64_t avail = n - static_cast<int64_t>(s) * block;
  return avail <= 0 ? 0 : (avail < block ? avail : block);
}

// The constructor's slot rounding (4 KiB) and slab size (one hipIpcOpenMemHandle can map).
int64_t sdma_slot_bytes(int64_t requested);
int64_t sdma_slab_bytes(int world, int64_t slot_bytes);
// Elements of `es` bytes one segment carries.
int64_t sdma_segment_elems(int world, int64_t slot_bytes, int64_t es);

// elements: the segment, block per rank, pipeline piece (4 KiB aligned); pieces of a block
struct SdmaSegment {
  int64_t n = 0, block = 0, pe = 0;
  int K = 1;
  int pieces_of(int j) const { return static_cast<int>((sdma_block_len(n, block, j) + pe - 1) / pe); }
  int64_t piece_len(int j, int k) const { return sdma_block_len(sdma_block_len(n, block, j), pe, k); }
};
// The same on every rank (n and world alone). pieces: 0 = by size. Throws
// std::logic_error("SdmaComm: segment exceeds the slot").
SdmaSegment plan_sdma_segment(int world, int64_t n, int64_t es, int64_t slot_bytes, int pieces);

// THE split of a byte range over `epp` engines: `count` parts of `size` bytes (4 KiB aligned;
// the last one shorter), part p on engine p.
struct SdmaParts {
  int64_t bytes = 0, size = 0;
  int count = 0;
  int64_t off(int p) const { return p * size; }
  int64_t len(int p) const { return bytes - off(p) < size ? bytes - off(p) : size; }
};
SdmaParts sdma_parts(int64_t bytes, int epp);

// Engines are single-bit ids of the device's mask, lowest first.
std::vector<uint32_t> sdma_engine_ids(uint32_t mask);
// connect_local: every `nloc`-th engine from `rank` on (0 = fewer engines than local ranks).
uint32_t sdma_engine_share(uint32_t local_engines, int nloc, int rank);
// engines_per_peer = 0: the rank's engines spread over its peers.
int sdma_auto_epp(int n_engines, int world);
// The `epp` engines towards peer k: those of `allowed` the direction's `avail_mask` names
// (none: all of `allowed`), dealt round-robin from k * epp.
std::vector<uint32_t> sdma_pick_engines(uint32_t avail_mask, uint32_t allowed, int k, int epp);

enum class SdmaSrc : uint8_t { In, Out, Epoch };  // the segment's input / output, the call's epoch word
enum class SdmaSig : uint8_t { Start, Mid, C1, C2, Scf, Gdf };
struct SdmaSigRef {
  SdmaSig kind = SdmaSig::Start;
  int index = 0;  // Mid, C2: k; C1: j * K + k
};
// One engine copy: `bytes` from the source to `dst_off` of rank `dst_rank`'s slab, queued on
// engine `engine` of those towards `peer`, started by `dep` reaching 0, decrementing `done`.
struct SdmaCopy {
  int dst_rank = 0;
  int64_t dst_off = 0;
  SdmaSrc src = SdmaSrc::In;
  int64_t src_off = 0, bytes = 0;
  SdmaSigRef dep, done;
  int peer = 0, engine = 0;
};
// Every signal is armed to the number of copies that complete into it (counted from the list).
struct SdmaSchedule {
  std::vector<int> c1, c2;  // [j * K + k], [k]
  int scf = 0, gdf = 0;
  std::vector<SdmaCopy> copies;  // in submission order
};
// One rank's copies of one segment. The order is part of the contract: an engine runs its
// queue in order, so
//   phase 1 (piece-major, then peer j): the parts of piece k of block j -> rank j's
//     SD[par][rank], each after `start`; then FS[rank][k] after c1[j,k], on the engine of the
//     piece's last part;
//   phase 2 (piece k of the own block): its parts -> every peer's RD[par][rank], each after
//     mid[k]; then - only after ALL of them are queued, a flag waits in its engine's queue for
//     every part of the piece - FR[rank][k] to every peer and to the own slab, after c2[k].
// `scratch` lends its vectors' capacity.
SdmaSchedule plan_sdma_copies(const SdmaSegment& seg, int world, int rank, int64_t es, int epp, int64_t slot_bytes,
                              int par, SdmaSchedule scratch = SdmaSchedule());

}  // namespace mxar
