#include "plane_group.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <thread>

#include "../core/data_buffer.h"
#include "../core/log.h"
#include "residency.h"

namespace mxar {

namespace {

std::atomic<uint32_t> g_res_gen{0};
std::atomic<int> g_group_teardown{0};

// Pinned state words of plane groups (64 B each) from blocks that are never freed: freeing
// pinned memory may synchronise the device while a co-located kernel spins.
std::mutex g_gword_mu;
std::vector<uint32_t*> g_gword_free;

uint32_t* take_group_word() {
  std::lock_guard<std::mutex> g(g_gword_mu);
  if (g_gword_free.empty()) {
    uint32_t* blk = nullptr;
    hip_check(hipHostMalloc(reinterpret_cast<void**>(&blk), 64 * 256, hipHostMallocCoherent | hipHostMallocMapped),
              "hipHostMalloc(group words)");
    std::memset(blk, 0, 64 * 256);
    for (int i = 255; i >= 0; --i) g_gword_free.push_back(blk + 16 * i);
  }
  uint32_t* w = g_gword_free.back();
  g_gword_free.pop_back();
  return w;
}

void give_group_word(uint32_t* w) {
  std::lock_guard<std::mutex> g(g_gword_mu);
  g_gword_free.push_back(w);
}

std::mutex g_group_mu;
std::map<std::string, std::weak_ptr<PlaneGroup>> g_groups;

}  // namespace

uint32_t next_resident_generation() { return g_res_gen.fetch_add(1) + 1u; }
int group_teardown_stage() { return g_group_teardown.load(); }

PlaneGroup::PlaneGroup(std::string k, int dev, int workers, bool high_priority) : key(std::move(k)), device(dev) {
  state.assign(static_cast<size_t>(workers), kPending);
  members.assign(static_cast<size_t>(workers), GroupMember());
  in_kernel.assign(static_cast<size_t>(workers), 0);
  hip_check(hipSetDevice(device), "hipSetDevice");
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  hip_check(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, high_priority ? hi : lo),
            "hipStreamCreate(plane group)");
  gword = take_group_word();
  reinterpret_cast<volatile uint32_t*>(gword)[0] = kResExited;
  hip_check(hipHostGetDevicePointer(reinterpret_cast<void**>(&gword_dev), gword, 0), "hipHostGetDevicePointer(group)");
  hip_check(hipMallocAsync(reinterpret_cast<void**>(&gdm), 64, stream), "hipMallocAsync(group words)");
  hip_check(hipMemsetAsync(gdm, 0, 64, stream), "hipMemsetAsync(group words)");
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize(group)");
}

PlaneGroup::~PlaneGroup() {
  // every worker left: the dispatcher saw each one's STOP (or no kernel ran)
  const volatile uint32_t* g = gword;
  g_group_teardown.store(1);
  const auto t0 = std::chrono::steady_clock::now();
  while (launched && g[0] != kResExited && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10))
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  (void)hipSetDevice(device);
  const bool exited = !launched || g[0] == kResExited;
  if (exited) {
    g_group_teardown.store(2);
    (void)hipStreamSynchronize(stream);
    g_group_teardown.store(3);
    for (auto& m : orphans) m->release();
  } else if (!orphans.empty()) {
    MXAR_LOG(ERROR, "plane", "group kernel still running at teardown: " << orphans.size()
                                                                          << " workers' round memory leaked");
    // never freed under a running kernel (a free synchronises the device, and the kernel still
    // polls these words): ownership is given up before `orphans` is destroyed
    for (auto& m : orphans) m->leak();
  }
  (void)hipFreeAsync(gdm, stream);
  (void)hipStreamDestroy(stream);
  if (exited) give_group_word(gword);  // else leaked: a kernel may still write it
  g_group_teardown.store(0);
}

void PlaneGroup::launch_locked(int by) {
  std::vector<XgmiComm*> comms;
  std::vector<const XgmiComm::ResidentPlan*> plans;
  std::vector<GroupResidentMember> mem;
  double idle_us = 1000.0;
  for (size_t k = 0; k < members.size(); ++k) {
    in_kernel[k] = 0;
    if (state[k] != kJoined) continue;
    const GroupMember& p = members[k];
    comms.push_back(p.comm);
    plans.push_back(p.plan);
    GroupResidentMember m = p.words;
    m.seq0 = *p.consumed + 1u;  // its first entry not consumed yet
    mem.push_back(m);
    in_kernel[k] = 1;
    idle_us = p.resident_idle_us;
  }
  if (comms.empty()) return;
  reinterpret_cast<volatile uint32_t*>(gword)[0] = kResRunning;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  try {
    XgmiComm::launch_group_resident(comms, plans, mem, gword_dev, gdm, next_resident_generation(),
                                    static_cast<uint64_t>(idle_us * 100.0), stream);
  } catch (...) {
    reinterpret_cast<volatile uint32_t*>(gword)[0] = kResExited;
    std::fill(in_kernel.begin(), in_kernel.end(), 0);
    throw;
  }
  launched = true;
  ++*members[static_cast<size_t>(by)].group_launches;
}

void PlaneGroup::ensure(int k, bool partial, double timeout_s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    {
      std::lock_guard<std::mutex> g(mu);
      if (kernel_left()) {
        const bool waiting = std::find(state.begin(), state.end(), kPending) != state.end();
        if (waiting && !partial) return;
        launch_locked(k);
        return;
      }
      if (in_kernel[static_cast<size_t>(k)]) return;  // running (or deciding to leave: it re-reads the doors)
    }
    if (std::chrono::steady_clock::now() - t0 > std::chrono::duration<double>(2 * timeout_s + 5))
      throw ProtocolError("xgmi plane group: a kernel without this worker never left");
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

std::shared_ptr<PlaneGroup> find_plane_group(const std::string& key, int device, int workers, bool high_priority,
                                             int reserve_wgs) {
  std::lock_guard<std::mutex> lk(g_group_mu);
  for (auto it = g_groups.begin(); it != g_groups.end();) it = it->second.expired() ? g_groups.erase(it) : std::next(it);
  auto& w = g_groups[key];
  std::shared_ptr<PlaneGroup> g = w.lock();
  if (!g) {
    g = std::make_shared<PlaneGroup>(key, device, workers, high_priority);
    if (reserve_wgs > 0)  // the dispatcher wave + every slice (throws with the budget named)
      g->residency = Residency::get().reserve(device, reserve_wgs, "plane group " + key);
    w = g;
  }
  return g;
}

}  // namespace mxar
