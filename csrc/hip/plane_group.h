// PlaneGroup: the co-located workers of one membership (this process, this GPU, one
// InitWorkers epoch). ONE resident kernel runs all their rounds, worker k's on its own slice
// of workgroups, fed from k's door ring (xgmi_threshold.hip threshold_group_resident_kernel).
// Found by key (device, the workers' arena ids in rank order, the membership epoch), so every
// worker of the membership joins the same group and a new membership forms a new one. The
// kernel runs while any worker has rounds; it leaves after an idle spell (the dispatcher
// decides for the whole group) and the next post launches it again. It is launched only once
// every worker has joined (its slices need every worker's words) - except for rounds being
// abandoned.
#pragma once

#include <hip/hip_runtime_api.h>

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "plane_memory.h"
#include "xgmi_comm.h"

namespace mxar {

// What a joined plane lends the group kernel (the plane keeps all of it alive while joined).
struct GroupMember {
  const void* owner = nullptr;  // the plane (identity only)
  XgmiComm* comm = nullptr;
  const XgmiComm::ResidentPlan* plan = nullptr;  // the group kernel's geometry for its slice
  GroupResidentMember words{};                   // door, state, device and force / abort words (seq0: at launch)
  const volatile uint32_t* consumed = nullptr;   // the last door entry a kernel consumed for it
  double resident_idle_us = 1000.0;
  uint64_t* group_launches = nullptr;  // its counter of group kernels it launched
};

struct PlaneGroup {
  enum : int { kPending = 0, kJoined = 1, kLeft = 2 };
  std::string key;
  int device = 0;
  std::vector<int> state;                 // per worker
  std::vector<GroupMember> members;       // joined workers
  std::vector<char> in_kernel;            // served by the kernel launched last
  uint32_t* gword = nullptr;              // pinned: [0] the kernel's state (kResRunning / ...)
  uint32_t* gword_dev = nullptr;
  uint64_t* gdm = nullptr;                // device words: [0] the dispatcher's heartbeat
  hipStream_t stream = nullptr;
  bool launched = false;                  // a kernel was launched (gword[0] says whether it left)
  // memory of workers whose STOP the kernel never took (XgmiRoundPlane::leave_group): the
  // kernel may still poll their doors and words, so it is freed only once the kernel is
  // known to have exited - or never (leaked) if it did not
  std::vector<std::shared_ptr<PlaneMemory>> orphans;
  std::shared_ptr<void> residency;  // the group kernel's workgroups in the device budget (residency.h)
  std::mutex mu;

  PlaneGroup(std::string k, int dev, int workers, bool high_priority);
  ~PlaneGroup();
  volatile uint32_t* state_word() const { return gword; }
  bool kernel_left() const { return !launched || reinterpret_cast<volatile uint32_t*>(gword)[0] == kResExited; }
  // Launches a kernel for every joined worker, on behalf of worker `by` (mu held; no kernel running).
  void launch_locked(int by);
  // Worker k posted an entry: make sure a kernel takes it. A kernel launched before k joined
  // does not serve k: wait for it to leave (bounded), then launch one that does. With workers
  // still to join, the last of them launches it - unless `partial` (k's rounds are being
  // abandoned: they must run now, without the missing worker).
  void ensure(int k, bool partial, double timeout_s);
};

// The group of the membership `key`, formed by the first of its workers to ask. reserve_wgs > 0:
// the new group reserves that many workgroups in the device budget (throws with the budget named).
std::shared_ptr<PlaneGroup> find_plane_group(const std::string& key, int device, int workers, bool high_priority,
                                             int reserve_wgs);
// Resident kernel generations, process-wide: a plane's device words (go = gen << 32 | seq)
// serve its own resident kernels and its group's in turn, and a kernel must never take a go
// that an earlier kernel of either kind wrote for the same entry (its STOP at an idle exit).
uint32_t next_resident_generation();
// where the last group teardown of this process is (debug_state while a configure leaves a
// group): 1 waiting for the kernel to leave, 2 synchronising its stream, 3 freeing orphans, 0 done
int group_teardown_stage();

}  // namespace mxar
