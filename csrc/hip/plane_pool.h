// OutputPool: an XgmiRoundPlane's round outputs and staging buffers. Round outputs come from
// a pool of equal-sized buffers (no allocator call on the round path); a dropped output
// returns to it at once on the plane stream, or - once exported to another stream - only
// behind the default stream (Shared::release_output, plane_pool.cc).
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <deque>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace mxar {

class OutputPool {
 public:
  // pool_grown / resident_pool_misses: the owner's counters (XgmiPlaneStats)
  OutputPool(hipStream_t stream, bool order_release, uint64_t* pool_grown, uint64_t* resident_pool_misses);
  // the plane stream is idle; frees the pooled buffers (outputs still held by users are freed
  // stream-ordered when dropped)
  ~OutputPool();
  // the owner is going: a buffer dropped from now on no longer returns to the pool
  void retire() { sh_->alive.store(false); }

  // Stream-ordered device buffer (hipMallocAsync on the plane stream, hipFreeAsync when the
  // last holder drops it): the launch path never calls a device-synchronising allocator
  // while a peer's kernel may be spinning on this worker's next launch.
  std::shared_ptr<void> buffer(size_t bytes, bool user_visible = false);
  // The same on the side stream: an idle stream of normal priority (never queued behind a
  // resident or group kernel's high-priority queue), created at first use.
  std::shared_ptr<void> side_buffer(size_t bytes);
  hipStream_t side_stream();
  // A round output from the pool, `*exported` its export flag.
  std::shared_ptr<void> out_buffer(size_t bytes, std::shared_ptr<std::atomic<bool>>* exported);
  // A pooled output for a round a resident or group kernel runs: nothing may queue on the
  // plane stream behind that kernel. null: the pool's growth was not ready in time (the round
  // takes the launch path). wait: a grouped worker has no launch path - it waits for the growth.
  std::shared_ptr<void> resident_out(size_t bytes, std::shared_ptr<std::atomic<bool>>* exported, bool wait = false);
  // A new membership: outputs of `bytes`, the pool grown now (resident_size: every round draws
  // from it, so it keeps more).
  void reset(size_t bytes, bool resident_size);
  // Before a launch: the exported outputs released since the last one become reusable behind
  // one default-stream event the plane stream waits for.
  void flush_releases();

 private:
  struct Shared {  // outlives the pool while a buffer's deleter may still look for it
    std::mutex mu;
    std::vector<void*> ptrs;  // released after an export: reusable once behind the default stream
    std::vector<void*> free;  // reusable now (ordered on the plane stream)
    size_t bytes = 0;         // size of the pooled output buffers
    std::atomic<bool> alive{true};
    hipStream_t stream = nullptr;
    bool ordered = true;
    void reuse_on_plane_stream(void* q) { free.push_back(q); }
    void reuse_behind_default_stream(void* q) { ptrs.push_back(q); }
    void release_output(void* q, size_t size, bool exported);
  };
  std::shared_ptr<Shared> sh_ = std::make_shared<Shared>();
  hipStream_t stream_;
  hipStream_t side_ = nullptr;
  hipEvent_t rel_ev_ = nullptr;
  // exported outputs released while a resident kernel holds the plane stream: reusable once
  // an event recorded on the default stream behind them has completed (host query)
  std::deque<std::pair<hipEvent_t, std::vector<void*>>> rel_pend_;
  std::vector<hipEvent_t> rel_spare_;
  uint64_t* pool_grown_;
  uint64_t* resident_pool_misses_;
};

}  // namespace mxar
