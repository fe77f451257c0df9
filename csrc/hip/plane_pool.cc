#include "plane_pool.h"

#include <algorithm>
#include <chrono>
#include <string>

#include "../core/env.h"
#include "xgmi_comm.h"

namespace mxar {

OutputPool::OutputPool(hipStream_t stream, bool order_release, uint64_t* pool_grown, uint64_t* resident_pool_misses)
    : stream_(stream), pool_grown_(pool_grown), resident_pool_misses_(resident_pool_misses) {
  sh_->stream = stream;
  sh_->ordered = order_release;
  hip_check(hipEventCreateWithFlags(&rel_ev_, hipEventDisableTiming), "hipEventCreate(release)");
}

OutputPool::~OutputPool() {
  retire();
  {
    std::lock_guard<std::mutex> g(sh_->mu);
    if (!sh_->ptrs.empty()) (void)hipStreamSynchronize(nullptr);
    for (void* q : sh_->ptrs) (void)hipFree(q);
    for (void* q : sh_->free) (void)hipFree(q);
    sh_->ptrs.clear();
    sh_->free.clear();
    sh_->bytes = 0;
  }
  if (rel_ev_) (void)hipEventDestroy(rel_ev_);
  for (auto& [ev, v] : rel_pend_) {
    (void)hipEventDestroy(ev);
    for (void* q : v) (void)hipFree(q);
  }
  for (hipEvent_t ev : rel_spare_) (void)hipEventDestroy(ev);
  if (side_) (void)hipStreamDestroy(side_);
}

// a dropped round output of `size` bytes: the two release rules
void OutputPool::Shared::release_output(void* q, size_t size, bool exported) {
  std::lock_guard<std::mutex> g(mu);
  if (bytes == size) {
    // exported: another stream may still read it - reusable only behind the default stream
    // (flush_releases at the next launch); otherwise at once, on the plane stream
    if (ordered && exported)
      reuse_behind_default_stream(q);
    else
      reuse_on_plane_stream(q);
    return;
  }
  // an output of an older layout: freed, stream-ordered behind whoever may still read it
  (void)hipFreeAsync(q, ordered && exported ? nullptr : stream);
}

std::shared_ptr<void> OutputPool::buffer(size_t bytes, bool user_visible) {
  void* p = nullptr;
  hip_check(hipMallocAsync(&p, std::max<size_t>(bytes, 256), stream_), "hipMallocAsync(plane)");
  // released on the plane stream (ordered after every round that may still read it); an
  // output the user keeps past the plane's lifetime is freed synchronously instead.
  // A round output went to the dataSink as a tensor: work the sink queued on the default
  // stream (torch's, e.g. a clone) may still read it when the last reference drops, so its
  // release is also ordered after the default stream - otherwise the next round could get
  // the same block from the pool and overwrite it under that work.
  static const bool via_event = [] {
    const char* e = study_env("MXAR_PLANE_RELEASE");
    return e != nullptr && std::string(e) == "event";
  }();
  return std::shared_ptr<void>(p, [w = std::weak_ptr<Shared>(sh_), user_visible](void* q) {
    auto r = w.lock();
    if (!r || !r->alive.load()) {
      // the plane is gone: stream-ordered on the default stream - hipFree would wait for
      // every kernel on the device, e.g. another plane's round spinning on its peers
      // (profiles/round2/sync_probe.md)
      (void)hipFreeAsync(q, nullptr);
    } else if (!user_visible) {
      (void)hipFreeAsync(q, r->stream);
    } else if (!via_event) {
      // freed on the default stream itself: ordered after whatever the sink queued there, and
      // the stream-ordered pool orders a later reuse by the plane stream after that free - no
      // event or stream wait on the launch path
      (void)hipFreeAsync(q, nullptr);
    } else {  // MXAR_PLANE_RELEASE=event: freed by the next launch, behind an event
      std::lock_guard<std::mutex> g(r->mu);
      r->reuse_behind_default_stream(q);
    }
  });
}

hipStream_t OutputPool::side_stream() {
  if (side_ == nullptr) hip_check(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking), "hipStreamCreate(plane side)");
  return side_;
}

std::shared_ptr<void> OutputPool::side_buffer(size_t bytes) {
  const hipStream_t ss = side_stream();
  void* p = nullptr;
  hip_check(hipMallocAsync(&p, std::max<size_t>(bytes, 256), ss), "hipMallocAsync(plane staging)");
  return std::shared_ptr<void>(p, [ss](void* q) { (void)hipFreeAsync(q, ss); });
}

std::shared_ptr<void> OutputPool::out_buffer(size_t bytes, std::shared_ptr<std::atomic<bool>>* exported) {
  bytes = std::max<size_t>(bytes, 256);
  void* p = nullptr;
  {
    std::lock_guard<std::mutex> g(sh_->mu);
    if (sh_->bytes == bytes && !sh_->free.empty()) {
      p = sh_->free.back();
      sh_->free.pop_back();
    }
  }
  if (p == nullptr) {
    hip_check(hipMallocAsync(&p, bytes, stream_), "hipMallocAsync(plane output)");
    ++*pool_grown_;
  }
  auto flag = std::make_shared<std::atomic<bool>>(false);
  *exported = flag;
  return std::shared_ptr<void>(p, [w = std::weak_ptr<Shared>(sh_), flag, bytes](void* q) {
    auto r = w.lock();
    if (r && r->alive.load()) return r->release_output(q, bytes, flag->load(std::memory_order_relaxed));
    // the plane is gone: stream-ordered on the default stream - hipFree would wait for every
    // kernel on the device, e.g. another plane's round spinning on its peers
    (void)hipFreeAsync(q, nullptr);
  });
}

void OutputPool::reset(size_t bytes, bool resident_size) {
  bytes = std::max<size_t>(bytes, 256);
  std::vector<void*> fr, pend;
  {
    std::lock_guard<std::mutex> g(sh_->mu);
    if (sh_->bytes == bytes) return;
    fr.swap(sh_->free);
    pend.swap(sh_->ptrs);
    sh_->bytes = bytes;
  }
  for (void* q : fr) (void)hipFreeAsync(q, stream_);
  for (void* q : pend) (void)hipFreeAsync(q, nullptr);
  // about 3 outputs are live at once (the round in flight, the one a sink holds, the one
  // being released): grow the pool now - growing it on the round path costs ~8 ms per
  // 256 MiB buffer (profiles/round2/sync_probe.md)
  // (resident-size rounds - every round then draws from this pool, see resident_out - keep
  // more: a sink holding a few outputs must not push rounds off the resident kernel)
  std::vector<void*> warm(resident_size ? 8 : 3, nullptr);
  for (void*& w : warm) hip_check(hipMallocAsync(&w, bytes, stream_), "hipMallocAsync(pool)");
  std::lock_guard<std::mutex> g(sh_->mu);
  for (void* w : warm) sh_->free.push_back(w);
}

void OutputPool::flush_releases() {
  std::vector<void*> ptrs;
  {
    std::lock_guard<std::mutex> g(sh_->mu);
    ptrs.swap(sh_->ptrs);
  }
  // releases parked by resident rounds: their events were recorded on the default stream
  // before the one below, so its wait covers them
  for (auto& [ev, v] : rel_pend_) {
    ptrs.insert(ptrs.end(), v.begin(), v.end());
    rel_spare_.push_back(ev);
  }
  rel_pend_.clear();
  if (ptrs.empty()) return;
  // one event for every exported output released since the last launch: their reuse by
  // this and later launches comes after everything the default stream held at this point -
  // e.g. a sink's clone of the round output
  hip_check(hipEventRecord(rel_ev_, nullptr), "hipEventRecord(release)");
  hip_check(hipStreamWaitEvent(stream_, rel_ev_, 0), "hipStreamWaitEvent(release)");
  std::lock_guard<std::mutex> g(sh_->mu);
  for (void* q : ptrs) sh_->free.push_back(q);
}

std::shared_ptr<void> OutputPool::resident_out(size_t bytes, std::shared_ptr<std::atomic<bool>>* exported, bool wait) {
  bytes = std::max<size_t>(bytes, 256);
  std::vector<void*> ptrs;
  {
    std::lock_guard<std::mutex> g(sh_->mu);
    if (sh_->bytes != bytes) return nullptr;
    ptrs.swap(sh_->ptrs);
  }
  if (!ptrs.empty()) {  // exported outputs: reusable behind what the default stream holds now
    hipEvent_t ev = nullptr;
    if (!rel_spare_.empty()) {
      ev = rel_spare_.back();
      rel_spare_.pop_back();
    } else {
      hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate(release)");
    }
    hip_check(hipEventRecord(ev, nullptr), "hipEventRecord(release)");
    rel_pend_.emplace_back(ev, std::move(ptrs));
  }
  while (!rel_pend_.empty()) {
    const hipError_t q = hipEventQuery(rel_pend_.front().first);
    if (q != hipSuccess) {
      (void)hipGetLastError();  // hipErrorNotReady is sticky-free, but keep the error state clean
      break;
    }
    std::lock_guard<std::mutex> g(sh_->mu);
    for (void* p : rel_pend_.front().second) sh_->free.push_back(p);
    rel_spare_.push_back(rel_pend_.front().first);
    rel_pend_.pop_front();
  }
  bool empty = false;
  {
    std::lock_guard<std::mutex> g(sh_->mu);
    empty = sh_->free.empty();
  }
  if (empty) {
    // Grow the pool with pool memory (hipMallocAsync) on the plane's idle side stream: the
    // kernel already running on the plane stream may use it once that stream has passed
    // the allocation - never a plain hipMalloc, whose later hipFreeAsync would fall back to a
    // device-wide synchronous free (the hazard for co-located planes' spinning kernels; ADVICE
    // r4). If the side stream does not get there within 100 us (it shares a hardware
    // queue with busy work), this round takes the launch path instead - no host wait on
    // another plane's kernel. reset() pre-grows resident-size pools, so this is rare.
    void* p = nullptr;
    const hipStream_t ss = side_stream();
    hip_check(hipMallocAsync(&p, bytes, ss), "hipMallocAsync(plane output)");
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t q;
    while ((q = hipStreamQuery(ss)) == hipErrorNotReady &&
           std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(100))
      __builtin_ia32_pause();
    (void)hipGetLastError();
    // a grouped worker has no launch path: it waits (the side stream has normal priority,
    // never behind the group kernel's queue)
    if (q == hipErrorNotReady && wait) q = hipStreamSynchronize(ss);
    std::lock_guard<std::mutex> g(sh_->mu);
    sh_->free.push_back(p);  // usable by the launch path in any case (stream-ordered after it)
    ++*pool_grown_;
    if (q != hipSuccess) {
      ++*resident_pool_misses_;
      return nullptr;
    }
  }
  return out_buffer(bytes, exported);
}

}  // namespace mxar
