#include "plane_door.h"

#include "../core/data_buffer.h"

namespace mxar {

uint32_t DoorRing::write(const ResidentDoor& e) {
  const uint32_t seq = seq_++;
  ResidentDoor* d = m_->door + seq % kResidentDoors;
  d->in = e.in;
  d->out = e.out;
  d->counts = e.counts;
  d->counts_host = e.counts_host;
  d->err_out = e.err_out;
  d->done_out = e.done_out;
  d->epoch = e.epoch;
  d->cmd = e.cmd;
  d->check = door_check(reinterpret_cast<const uint32_t*>(&e), seq);
  __atomic_store_n(&d->seq, seq, __ATOMIC_RELEASE);  // sequence word last
  return seq;
}

bool DoorRing::post(const ResidentDoor& e, const volatile uint32_t* state) {
  const volatile uint32_t* sw = state != nullptr ? state : m_->rstate;
  // the door slot is free once the kernel consumed the entry kResidentDoors before this one
  // (rounds in flight are bounded by the ring's slots, so this does not wait in practice)
  const auto t0 = std::chrono::steady_clock::now();
  while (static_cast<int32_t>(seq_ - static_cast<uint32_t>(kResidentDoors) - m_->rstate[1]) > 0 &&
         sw[0] != kResExited) {
    if (std::chrono::steady_clock::now() - t0 > bound_) {
      ++seq_;  // the entry's number is spent, as if it had been written
      throw ProtocolError("xgmi plane: the resident round kernel stopped taking rounds");
    }
    __builtin_ia32_pause();
  }
  write(e);
  // Dekker hand-off with the kernel's idle exit (xgmi_threshold.hip, resident_door): the
  // entry is visible before the state word is read
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  uint32_t st = sw[0];
  while (st == kResExiting) {
    if (std::chrono::steady_clock::now() - t0 > bound_)
      throw ProtocolError("xgmi plane: the resident round kernel neither took nor refused a round");
    __builtin_ia32_pause();
    st = sw[0];
  }
  return st != kResExited;
}

void DoorRing::start_at(uint32_t seq) {
  m_->rstate[1] = seq - 1u;
  m_->rstate[0] = kResRunning;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
}

}  // namespace mxar
