// DoorRing: the host side of the door protocol between an XgmiRoundPlane and the resident
// kernel that runs its rounds - its own (threshold_resident_kernel) or its group's
// (threshold_group_resident_kernel), xgmi_threshold.hip resident_door. The plane writes
// numbered entries (rounds, STOP) into a pinned ring; the kernel polls the ring, publishes
// the last entry it consumed in rstate[1] and its own state in a state word (rstate[0] for
// the plane's kernel, the group's word for a group kernel).
#pragma once

#include <chrono>
#include <thread>

#include "plane_memory.h"

namespace mxar {

class DoorRing {
 public:
  // mem outlives the ring; timeout_s: the plane's round timeout (the waits below are bounded
  // by 2 x timeout_s + 5 s: the kernel bounds its own waits by timeout_s)
  void bind(const PlaneMemory* mem, double timeout_s) {
    m_ = mem;
    bound_ = std::chrono::duration<double>(2 * timeout_s + 5);
  }
  uint32_t next() const { return seq_; }              // the next entry's number
  uint32_t consumed() const { return m_->rstate[1]; }  // the last entry a kernel consumed
  const ResidentDoor& last() const { return m_->door[(seq_ - 1u) % kResidentDoors]; }
  // The one writer of a door entry: fills slot next(), its check word, and release-stores the
  // sequence word last. Returns the entry's number.
  uint32_t write(const ResidentDoor& e);
  // Writes entry next() and hands it to the kernel; false = the kernel had exited before it
  // took the entry (nothing runs it). state: the kernel's state word (null: rstate[0]).
  bool post(const ResidentDoor& e, const volatile uint32_t* state = nullptr);
  // A fresh kernel starts at entry seq: everything before counts as consumed, the state word
  // says running before the launch.
  void start_at(uint32_t seq);
  // Posts a STOP entry behind the posted rounds and waits until done(seq of the STOP), polling
  // every nap_us (0: yield). false: the bound passed first (the caller logs what that means).
  template <class Done>
  bool stop_and_wait(const volatile uint32_t* state, Done done, int nap_us) {
    ResidentDoor e{};
    e.cmd = kResStop;
    const uint32_t seq = seq_;
    if (!post(e, state)) return true;  // it had left already
    const auto t0 = std::chrono::steady_clock::now();
    while (!done(seq)) {
      if (std::chrono::steady_clock::now() - t0 > bound_) return false;
      if (nap_us > 0)
        std::this_thread::sleep_for(std::chrono::microseconds(nap_us));
      else
        std::this_thread::yield();
    }
    return true;
  }
  // every entry before next() was taken or is dropped: no kernel launched later takes it
  void drop_unconsumed() { m_->rstate[1] = seq_ - 1u; }
  // entries posted that no kernel consumed yet
  bool pending() const { return static_cast<int32_t>(seq_ - 1u - m_->rstate[1]) > 0; }

 private:
  const PlaneMemory* m_ = nullptr;
  std::chrono::duration<double> bound_{0};
  uint32_t seq_ = 1;  // next door entry
};

}  // namespace mxar
