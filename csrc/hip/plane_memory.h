// PlaneMemory: the one owner of an XgmiRoundPlane's device and pinned memory. Allocated once,
// for the largest membership the plane may see, and never reallocated: hipFree / hipHostFree
// in configure() could synchronise the device while a peer's round kernel spins waiting for
// this worker's re-initialisation. A plane whose group kernel never took its STOP moves the
// whole of it to the group (PlaneGroup::orphans), which frees it once that kernel is gone - or leaks it.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "comm_args.h"

namespace mxar {

// the words themselves: plain data, so the owner below moves and empties them as a block
struct PlaneWords {
  char* arena = nullptr;             // fine-grained HBM: the communicator's slabs and flags (IPC-exported)
  uint32_t* hforce = nullptr;        // pinned words the engine raises: [0] force, [1] abort
  uint32_t* hforce_dev = nullptr;    // their device-visible address
  int32_t* ring = nullptr;           // pinned ring: per slot P x nch counts, the done and the error word
  int32_t* ring_dev = nullptr;       // the ring's device-visible address
  int32_t* cnt_vram = nullptr;       // per-slot counts the workgroups write (HBM); copied into the ring at round end
  uint32_t* ctl = nullptr;           // the communicator's control words, kept across epochs
  ResidentDoor* door = nullptr;      // pinned door ring (kResidentDoors entries)
  ResidentDoor* door_dev = nullptr;  // its device-visible address
  volatile uint32_t* rstate = nullptr;  // pinned, behind the doors: [0] kernel state, [1] last entry it consumed
  uint32_t* rstate_dev = nullptr;
  uint32_t* rdm = nullptr;           // the resident kernel's device words
  void* split = nullptr;             // split-chunk scratch (XgmiComm::RoundSpec::split_scratch), zeroed per membership
  size_t split_bytes = 0;
  size_t ring_stride = 0;            // int32 per slot
};

struct PlaneMemory : PlaneWords {
  PlaneMemory() = default;
  // Every allocation zeroed (the arena ONCE, here, before anyone can know its handle: every
  // flag reads "epoch 0 done"); a throw part-way frees what exists. The device is current.
  PlaneMemory(int64_t arena_bytes, size_t ring_stride, int ring_slots, size_t split_bytes);
  PlaneMemory(PlaneMemory&& o) noexcept { *this = static_cast<PlaneMemory&&>(o); }
  PlaneMemory& operator=(PlaneMemory&& o) noexcept;
  PlaneMemory(const PlaneMemory&) = delete;
  PlaneMemory& operator=(const PlaneMemory&) = delete;
  ~PlaneMemory() { release(); }
  void release();  // frees everything (device-synchronising calls) and leaves this empty
  void leak() { static_cast<PlaneWords&>(*this) = PlaneWords(); }  // empty without freeing: a kernel still uses it
  explicit operator bool() const { return arena != nullptr; }

  // A ring slot's words. The kernel counts into the slot's HBM twin and copies the counts,
  // with the error and the done word, into the pinned slot at round end (no per-round D2H
  // copy); the host reads the pinned slot.
  int32_t* counts_dev(int slot) const { return cnt_vram + static_cast<size_t>(slot) * ring_stride; }
  int32_t* counts_host(int slot) const { return ring_dev + static_cast<size_t>(slot) * ring_stride; }
  uint32_t* err_word(int slot) const { return reinterpret_cast<uint32_t*>(counts_host(slot) + ring_stride - 1); }
  uint32_t* done_word(int slot) const { return reinterpret_cast<uint32_t*>(counts_host(slot) + ring_stride - 2); }
  // the host's view of the same slot (decode_slot, plane_rounds.h) and of its done word
  const volatile int32_t* slot_words(int slot) const { return ring + static_cast<size_t>(slot) * ring_stride; }
  const volatile uint32_t* done_seen(int slot) const {
    return reinterpret_cast<const volatile uint32_t*>(slot_words(slot) + ring_stride - 2);
  }
};

}  // namespace mxar
