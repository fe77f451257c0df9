#include "plane_memory.h"

#include <cstring>

#include "xgmi_comm.h"

namespace mxar {

PlaneMemory::PlaneMemory(int64_t arena_bytes, size_t stride, int ring_slots, size_t split_sz) {
  split_bytes = split_sz;
  ring_stride = stride;
  constexpr unsigned kPinned = hipHostMallocCoherent | hipHostMallocMapped;
  const size_t ring_bytes = ring_stride * 4 * static_cast<size_t>(ring_slots);
  const size_t door_bytes = sizeof(ResidentDoor) * kResidentDoors + 64;
  try {
    hip_check(hipExtMallocWithFlags(reinterpret_cast<void**>(&arena), arena_bytes, hipDeviceMallocFinegrained),
              "hipExtMallocWithFlags(plane arena)");
    hip_check(hipMemset(arena, 0, arena_bytes), "hipMemset(plane arena)");
    hip_check(hipHostMalloc(reinterpret_cast<void**>(&hforce), 64, kPinned), "hipHostMalloc(force word)");
    std::memset(hforce, 0, 64);
    hip_check(hipHostGetDevicePointer(reinterpret_cast<void**>(&hforce_dev), hforce, 0), "hipHostGetDevicePointer");
    hip_check(hipHostMalloc(reinterpret_cast<void**>(&ring), ring_bytes, kPinned), "hipHostMalloc(plane ring)");
    std::memset(ring, 0, ring_bytes);
    hip_check(hipHostGetDevicePointer(reinterpret_cast<void**>(&ring_dev), ring, 0), "hipHostGetDevicePointer(ring)");
    hip_check(hipMalloc(reinterpret_cast<void**>(&cnt_vram), ring_bytes), "hipMalloc(plane counts)");
    hip_check(hipMalloc(reinterpret_cast<void**>(&ctl), 256), "hipMalloc(plane ctl)");
    hip_check(hipHostMalloc(reinterpret_cast<void**>(&door), door_bytes, kPinned), "hipHostMalloc(resident door)");
    std::memset(door, 0, door_bytes);
    hip_check(hipHostGetDevicePointer(reinterpret_cast<void**>(&door_dev), door, 0), "hipHostGetDevicePointer(door)");
    rstate = reinterpret_cast<volatile uint32_t*>(door + kResidentDoors);
    rstate_dev = reinterpret_cast<uint32_t*>(door_dev + kResidentDoors);
    hip_check(hipMalloc(reinterpret_cast<void**>(&rdm), 256), "hipMalloc(resident words)");
    hip_check(hipMemset(rdm, 0, 256), "hipMemset(resident words)");
    hip_check(hipMemset(ctl, 0, 256), "hipMemset(plane ctl)");
    hip_check(hipMalloc(&split, split_bytes), "hipMalloc(plane split scratch)");
    hip_check(hipMemset(split, 0, split_bytes), "hipMemset(plane split scratch)");
  } catch (...) {
    release();
    throw;
  }
}

PlaneMemory& PlaneMemory::operator=(PlaneMemory&& o) noexcept {
  if (this == &o) return *this;
  release();
  static_cast<PlaneWords&>(*this) = o;
  static_cast<PlaneWords&>(o) = PlaneWords();
  return *this;
}

void PlaneMemory::release() {
  if (ring) (void)hipHostFree(ring);
  if (cnt_vram) (void)hipFree(cnt_vram);
  if (ctl) (void)hipFree(ctl);
  if (split) (void)hipFree(split);
  if (hforce) (void)hipHostFree(hforce);
  if (door) (void)hipHostFree(door);
  if (rdm) (void)hipFree(rdm);
  if (arena) (void)hipFree(arena);
  static_cast<PlaneWords&>(*this) = PlaneWords();
}

}  // namespace mxar
