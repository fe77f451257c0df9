// XgmiRoundPlane: the MI355X data plane of the round-granular protocol engine
// (PlaneWorkerActor, csrc/runtime/plane_worker.h). One persistent threshold-kernel launch
// per allreduce round (csrc/hip/xgmi_threshold.hip) replaces the reference's per-chunk
// ScatterBlock / ReduceBlock messages (AllreduceWorker.scala:194-251) with direct xGMI
// peer stores into the owners' HBM slots.
//
// The plane keeps its own decisions - configure (InitWorkers), which path a round takes, force /
// abort, the completion thread - and is built from parts (docs/ARCHITECTURE.md, "The
// protocol-driven round engine"): PlaneMemory (plane_memory.h: the arena, exported with
// hipIpcGetMemHandle in the descriptor, and every pinned / device word), OutputPool
// (plane_pool.h), DoorRing (plane_door.h), RoundQueue / decode_slot (runtime/plane_rounds.h),
// PlaneGroup (plane_group.h).
//   * configure: the reference's block ranges (step = ceil(N / P), float32) and maxChunkSize
//     chunks; an XgmiComm is laid out over the arena (rows = maxLag + 1) and connected to the
//     peers' arenas (IPC mappings kept across epochs; workers of one process find each
//     other's arenas through a process-local registry).
//   * launch (StartAllreduce), one of three paths, same round semantics and done word:
//     co-located workers (several workers of one job in this process on this GPU) run every
//     round in ONE resident group kernel, a slice of workgroups per worker fed from that
//     worker's door (no round waits in a hardware queue behind a co-located peer's spinning
//     round); a lone worker's rounds of <= resident_max bytes are posted to its own resident
//     kernel, which leaves after an idle spell or when the plane needs its stream; every other
//     round is one threshold launch with the round's explicit epoch
//     (roundBase + r - startRound + 1), its input ordered after its producer on the stream.
//     The kernel writes per-chunk counts, the error word and a done word to a pinned slot; the
//     completion thread hands each finished round to the worker in launch order.
//   * force (catch-up): raises a pinned host word the kernel polls; rounds <= it complete
//     with what has arrived. Peers ahead by more than maxLag force us through our slab.
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../core/trace.h"
#include "../runtime/plane_rounds.h"
#include "../runtime/round_plane.h"
#include "device_plane.h"
#include "plane_door.h"
#include "plane_group.h"
#include "plane_memory.h"
#include "plane_pool.h"
#include "xgmi_comm.h"

namespace mxar {

struct XgmiPlaneOptions {
  int device = 0;
  DType dtype = DType::F32;
  int64_t capacity = 0;  // elements per round (>= the job's dataSize)
  int max_peers = 8;     // largest membership the arena is sized for
  int max_lag = 4;       // largest maxLag the arena is sized for
  int grid = 0;          // workgroups per launch (0: 2 per CU; split when planes share a GPU)
  double timeout_s = 60.0;
  bool order_ref = true;  // the reference's arrival-order accounting (threshold kernel doc)
  int ring = 64;          // rounds in flight at most (pinned count / error slots)
  bool high_priority = true;  // plane stream priority (see XgmiRoundPlane ctor)
  bool order_release = true;  // a round output's release waits for the default stream (buffer())
  int spin_us = 1000;         // completion thread polls a round's event this long before blocking
  bool split = true;          // chunks fewer than workgroups are split over several (threshold kernel)
  // Smallest maxChunkSize (elements) that keeps one flag word, count and threshold decision
  // per reference chunk (DataBuffer.scala:12,28-29,69-75); 0 = 1 KiB of data per flag. Finer
  // chunks cost flag-table memory (3 x rows x P words per chunk). A job with a finer
  // maxChunkSize runs at thresholds 1 with chunks coarsened to the flag granularity (counts
  // reported per reference chunk), and is refused at thresholds < 1 (ProtocolError).
  int64_t min_chunk = 0;
  // Resident rounds of a lone worker (XgmiComm::launch_resident; co-located workers run every
  // round on their group kernel instead): rounds of at most this many bytes are posted
  // to a kernel that stays on the plane stream between rounds instead of one launch each
  // (0 = off; MXAR_PLANE_RESIDENT). The kernel leaves after `resident_idle_us` without a
  // round (MXAR_PLANE_RESIDENT_IDLE_US) and is launched again by the next one. Rounds whose
  // geometry needs more than 64 workgroups (MXAR_PLANE_RESIDENT_GRID) or split chunks are
  // launched. 2 workers, th 1, bench geometry: 256 KiB 38-47 -> 32-34 us, 1 MiB 44-45 ->
  // 34-40, 4 MiB 46-52 -> 42-47 per round (profiles/round4/resident_grid_ab.jsonl).
  int64_t resident_max = 4 << 20;
  // Lag skip (XgmiComm::RoundSpec::lag_wait_us): a round waits at most this long at its lag
  // gate for a peer still inside the round that last used the row, then runs without it
  // (writes nothing to it, forces it). < 0: wait for the peer - a straggler then holds every
  // fast worker within maxLag + 1 rounds of itself (bounded buffers). Applies only where
  // the thresholds let a round complete without one peer.
  double lag_wait_us = -1.0;
  // The owner reserved this plane's group-kernel workgroups in the device residency budget
  // (residency.h) already - PlaneJob does, for all its co-located planes at once, so a job that
  // cannot fit fails at construction. false: the group reserves them itself when it forms.
  bool residency_external = false;
  int resident_grid = 64;
  double resident_idle_us = 1000.0;
};

struct XgmiPlaneStats {
  uint64_t launches = 0, cold = 0, forced = 0, bytes = 0, completed = 0, coarsened = 0, peer_maps = 0;
  uint64_t pool_grown = 0;  // round outputs the pool had to allocate (none after warm-up in steady state)
  uint64_t resident_pool_misses = 0;  // resident-size rounds launched instead: pool growth not ready in time
  uint64_t resident_rounds = 0, resident_launches = 0, resident_parks = 0;
  uint64_t group_rounds = 0;   // rounds run by the co-located workers' group kernel
  uint64_t group_launches = 0;  // group kernels this worker launched
  int group_size = 0;          // co-located workers in the current membership (0: none / alone)
};

class XgmiRoundPlane final : public RoundPlane {
 public:
  explicit XgmiRoundPlane(const XgmiPlaneOptions& o);
  ~XgmiRoundPlane() override;
  const char* name() const override { return "xgmi"; }
  std::string descriptor() const override { return desc_; }
  void set_done(DoneFn fn) override;
  void configure(const PlaneConfig& cfg) override;
  void launch(int round, const Payload& input, bool cold) override;
  void force(int round) override;
  void abort(int round) override;
  void drain() override { rounds_.drain(); }
  // chunks per block as the reference counts them (ceil(block / maxChunkSize)): the length of
  // an output's counts is peers x chunks()
  int chunks() const override { return nch_ref_; }

  const XgmiPlaneOptions& options() const { return o_; }
  const XgmiPlaneStats& stats() const { return st_; }
  hipStream_t stream() const { return stream_; }
  int64_t arena_bytes() const { return arena_bytes_; }
  int64_t chunk_elems() const { return chunk_; }
  int64_t block_elems() const { return block_; }
  XgmiComm* comm() const { return comm_.get(); }
  // Diagnostics (blocking copies of device words - never on a hot path): the door / resident
  // words, the group's state, the device go word and control words.
  std::string debug_state() const;
  // Phase-stamp buffer for this plane's round kernels (study knob, XgmiComm::set_phase_stamps);
  // kept across re-initialisations. Call between rounds.
  void set_phase_stamps(uint64_t* buf, int64_t slots) {
    park_resident();  // a resident kernel holds the old launch arguments
    rplan_tried_ = false;
    stamps_ = buf;
    stamp_slots_ = buf ? slots : 0;
    if (comm_) comm_->set_phase_stamps(stamps_, stamp_slots_);
  }

 private:
  struct Rec {  // a round in flight
    int round = 0;
    int64_t epoch = 0;
    std::shared_ptr<void> out, staging;
    std::shared_ptr<std::atomic<bool>> exported;  // the output's export flag (OutputPool::out_buffer)
    uint32_t round_epoch = 0;                      // the kernel's round epoch (done word)
    Payload input;
    hipEvent_t ev = nullptr;
    int slot = 0;
    bool cold = false;
  };
  using Lease = RoundQueue<Rec>::SlotLease;
  enum class Path { Launched, Resident, Group };  // who runs a round
  uint32_t epoch_of(int round) const {
    return cfg_.roundBase + static_cast<uint32_t>(round - cfg_.startRound) + 1u;
  }
  size_t round_bytes() const { return static_cast<size_t>(cfg_.dataSize) * dtype_size(o_.dtype); }
  char* map_peer(const std::string& desc);
  void completion_loop();

  // One submission path (launch): the parts every path shares.
  XgmiComm::RoundSpec round_spec() const;      // the membership-wide fields of a round's spec
  Rec begin_round(int round, bool cold) const;  // the record fields every path fills alike
  ResidentDoor door_entry(const Rec& rec, const void* in_ptr) const;  // a posted round (resident, group)
  void submit(Rec&& rec, Lease& lease, Path path);  // bookkeeping tail: counters, queue, wake-up
  TraceScope round_span(const char* kind, const Rec& rec) const;
  // the payload as device memory of this GPU (null: a host or another device's payload)
  const DevicePayload* device_input(const Payload& input) const;
  // Has the payload's producer finished? If not, the host waits for it: budget_us < 0 for as
  // long as it takes (throws on a HIP error), else at most that long (false: not yet, or an error).
  bool producer_done(const DevicePayload& dp, int64_t budget_us) const;
  // Uploads a host payload / casts a device payload into the plane dtype on the plane stream
  // (side = false) or the pool's side stream, which is then waited for (side = true), with
  // buffers of that stream; rec keeps alive what the stream work reads. Returns the round's input.
  const void* stage_input(Rec& rec, const Payload& input, const DevicePayload* dp, bool side);
  // The three paths. Resident rounds: post the round to the resident kernel (launching it if
  // none runs); false = the round needs the launch path (park_resident first).
  void launch_group(int round, const Payload& input, bool cold);
  bool launch_resident(int round, const Payload& input, bool cold);
  void launch_stream(int round, const Payload& input, bool cold);
  // Stops the resident kernel (a STOP entry behind the posted rounds) and waits for it to leave.
  void park_resident();
  // Co-located workers (PlaneGroup): join the group of this membership (configure), leave it
  // (a STOP entry for this worker's slice; configure / destruction).
  void join_group(const PlaneConfig& cfg);
  void leave_group();
  // the workers of this membership in this process on this device: (rank, arena id)
  std::vector<std::pair<int, uint64_t>> colocated(const PlaneConfig& cfg) const;

  XgmiPlaneOptions o_;
  bool coarsen_full_ = true;    // MXAR_PLANE_COARSEN=0: kernel chunks = maxChunkSize at thresholds 1
  int wg_chunks_ = 1;           // at thresholds 1: kernel chunks per workgroup at most (0: no cap)
  int64_t arena_bytes_ = 0;
  int64_t flag_bytes_ = 0;  // flag table reserved at its largest size (every layout the same)
  int64_t flag_gran_ = 0;   // slot bytes per flag word (XgmiComm flag_gran)
  uint64_t arena_id_ = 0;
  std::string desc_;
  PlaneMemory mem_;                    // every device / pinned word of the plane (empty once orphaned)
  hipStream_t stream_ = nullptr;
  std::vector<hipEvent_t> events_;     // one per ring slot
  std::unique_ptr<OutputPool> pool_;   // round outputs and staging buffers
  DoorRing door_;                      // the door to the resident / group kernel
  RoundQueue<Rec> rounds_;             // ring slots and the rounds in flight, in launch order
  std::unique_ptr<XgmiComm> comm_;
  std::map<std::string, char*> mapped_;  // peer IPC handle -> mapping (kept across epochs)

  PlaneConfig cfg_;
  bool configured_ = false;
  // where configure() is (debug_state): 0 idle, 1 abandoning the old epoch's rounds, 2 draining
  // them, 3 leaving the old group (31-35: leave_group's steps), 4 parking a solo kernel, 5
  // mapping peers, 6 the new communicator and published progress, 7 joining the new group
  std::atomic<int> cfg_stage_{0};
  int64_t block_ = 0, chunk_ = 0;
  int nch_ = 0;       // chunks per block the kernel runs
  int nch_ref_ = 0;   // reference chunks per block (= nch_ unless coarsened at thresholds 1)
  int coarse_ = 1;    // reference chunks per kernel chunk
  int last_round_ = -1;  // last launched round of this epoch
  uint32_t err_seen_ = 0;
  uint64_t* stamps_ = nullptr;
  int64_t stamp_slots_ = 0;
  XgmiPlaneStats st_;

  // a lone worker's resident kernel
  XgmiComm::ResidentPlan rplan_;
  bool rplan_tried_ = false;
  std::shared_ptr<void> res_token_;    // the resident kernel's share of the residency budget
  bool res_on_ = false;                // a resident kernel was launched and may still run
  // co-located workers
  bool grouped_ = false;  // this membership has co-located workers (configure)
  // the group kernel never took this worker's STOP: its round memory went to the group
  // (PlaneGroup::orphans) and the plane can run no further round
  bool orphaned_ = false;
  std::shared_ptr<PlaneGroup> group_;
  int gidx_ = -1;                      // this worker's index in the group
  XgmiComm::ResidentPlan gplan_;       // the group kernel's geometry for this membership

  std::mutex done_mu_;
  DoneFn done_;
  std::thread th_;  // the completion thread: hands each finished round to the worker in launch order
};

std::shared_ptr<XgmiRoundPlane> make_xgmi_plane(const XgmiPlaneOptions& o);

}  // namespace mxar
