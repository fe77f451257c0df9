// The host bookkeeping of a round plane's rounds in flight (xgmi_plane.cc), free of HIP so it
// runs under the sanitizers without a GPU (csrc/tests/runtime_stress.cc, scenario "rounds"):
//   * RoundQueue: the ring's slot free-list and the FIFO between the launching thread and the
//     completion thread, with their lock-free hand-off;
//   * decode_slot: what a finished round left in its pinned slot (epoch-tagged counts, the
//     error word).
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <mutex>
#include <utility>
#include <vector>

namespace mxar {

template <class Rec>
class RoundQueue {
 public:
  // A slot taken for a round being submitted: goes back to the free list unless the round
  // was queued (commit) - whatever throws in between cannot leak it.
  class SlotLease {
   public:
    SlotLease(RoundQueue* q, int slot) : q_(q), slot_(slot) {}
    SlotLease(SlotLease&& o) noexcept : q_(std::exchange(o.q_, nullptr)), slot_(o.slot_) {}
    SlotLease(const SlotLease&) = delete;
    SlotLease& operator=(const SlotLease&) = delete;
    ~SlotLease() {
      if (q_ != nullptr) q_->release(slot_);
    }
    int slot() const { return slot_; }
    void commit() { q_ = nullptr; }

   private:
    RoundQueue* q_;
    int slot_;
  };

  // every slot of a ring of `ring` free again (no round in flight)
  void reset_slots(int ring) {
    std::lock_guard<std::mutex> g(mu_);
    free_.clear();
    for (int i = ring - 1; i >= 0; --i) free_.push_back(i);
  }
  // blocks while no slot is free (rounds in flight are bounded by the ring)
  SlotLease take_slot() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_idle_.wait(lk, [&] { return !free_.empty(); });
    const int s = free_.back();
    free_.pop_back();
    return SlotLease(this, s);
  }
  // Queues a submitted round. The consumer is polling for it unless it went to sleep (a futex
  // wake costs the launch path microseconds): notified only then.
  void push(Rec rec) {
    std::unique_lock<std::mutex> lk(mu_);
    q_.push_back(std::move(rec));
    len_.fetch_add(1, std::memory_order_release);
    lk.unlock();
    if (sleeping_.load(std::memory_order_seq_cst)) cv_.notify_all();
  }
  // The consumer's wait for the oldest round: the next one is usually submitted within
  // microseconds, so poll for it (spin_us) before sleeping on the condition variable. The
  // round stays queued until pop_and_release (drain waits for that). false: stopped and empty.
  bool wait_front(int spin_us, Rec* out) {
    const auto t_idle = std::chrono::steady_clock::now();
    const auto idle_budget = std::chrono::microseconds(spin_us);
    for (unsigned i = 0; len_.load(std::memory_order_acquire) == 0; ++i) {
      if ((i & 63) == 0 && (stop_flag_.load(std::memory_order_relaxed) ||
                            std::chrono::steady_clock::now() - t_idle > idle_budget))
        break;
      __builtin_ia32_pause();
    }
    std::unique_lock<std::mutex> lk(mu_);
    sleeping_.store(true, std::memory_order_seq_cst);
    cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
    sleeping_.store(false, std::memory_order_relaxed);
    if (q_.empty()) return false;
    *out = q_.front();
    return true;
  }
  // the oldest round is done (its callback ran): its slot is free, drain may return
  void pop_and_release(int slot) {
    {
      std::lock_guard<std::mutex> g(mu_);
      free_.push_back(slot);
      q_.pop_front();
      len_.fetch_sub(1, std::memory_order_relaxed);
    }
    cv_idle_.notify_all();
  }
  // returns once no round is queued
  void drain() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_idle_.wait(lk, [&] { return q_.empty(); });
  }
  // ends a consumer that polls or sleeps with nothing queued (wait_front returns false)
  void stop() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    stop_flag_.store(true);
    cv_.notify_all();
  }
  int size() const { return len_.load(); }
  int free_slots() {
    std::lock_guard<std::mutex> g(mu_);
    return static_cast<int>(free_.size());
  }

 private:
  void release(int slot) {
    {
      std::lock_guard<std::mutex> g(mu_);
      free_.push_back(slot);
    }
    cv_idle_.notify_all();
  }
  std::mutex mu_;
  std::condition_variable cv_, cv_idle_;
  std::deque<Rec> q_;
  std::vector<int> free_;
  std::atomic<int> len_{0};           // q_.size(), polled without the lock by the consumer
  std::atomic<bool> sleeping_{false};  // the consumer waits on cv_ (push must notify)
  std::atomic<bool> stop_flag_{false};
  bool stop_ = false;
};

// A round's pinned slot: `stride` words, [0, P x nch) the per-chunk counts, [stride - 2] the
// done word, [stride - 1] the error word. The kernel writes counts and error word after its
// last release, each as (round epoch & 0xffffff) << 8 | value (xgmi_threshold.hip host_tag),
// so they may land after the done word.
inline bool slot_tagged(const volatile int32_t* words, size_t i, uint32_t round_epoch) {
  return (static_cast<uint32_t>(words[i]) >> 8) == (round_epoch & 0xffffffu);
}
// every count from *from on (advanced past the tagged ones) and the error word carry this epoch's tag
inline bool slot_ready(const volatile int32_t* words, size_t stride, size_t counts, uint32_t round_epoch,
                       size_t* from) {
  while (*from < counts && slot_tagged(words, *from, round_epoch)) ++*from;
  return *from >= counts && slot_tagged(words, stride - 1, round_epoch);
}

struct SlotResult {
  std::vector<int32_t> count;  // P x nch_ref: per reference chunk
  uint32_t error = 0;          // the raw error byte
};

// What a slot that is ready holds. coarse > 1 (coarsened at thresholds 1): every reference chunk
// of a kernel chunk shares its count, count[j * nch_ref + c] = cnt[j * nch + c / coarse]
inline SlotResult decode_slot(const volatile int32_t* words, size_t stride, int P, int nch, int nch_ref, int coarse) {
  SlotResult r;
  auto cnt = [&](size_t i) { return static_cast<int32_t>(static_cast<uint32_t>(words[i]) & 0xffu); };
  if (coarse == 1) {
    r.count.resize(static_cast<size_t>(P) * nch);
    for (size_t i = 0; i < r.count.size(); ++i) r.count[i] = cnt(i);
  } else {
    r.count.resize(static_cast<size_t>(P) * nch_ref);
    for (int j = 0; j < P; ++j)
      for (int c = 0; c < nch_ref; ++c)
        r.count[static_cast<size_t>(j) * nch_ref + c] = cnt(static_cast<size_t>(j) * nch + c / coarse);
  }
  r.error = static_cast<uint32_t>(words[stride - 1]) & 0xffu;
  return r;
}

}  // namespace mxar
