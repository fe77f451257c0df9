// XgmiComm, host side: slab allocation and IPC, stream ordering, and one launch per segment.
// The kernels and their launchers live in the .hip files (xgmi_launch.h); every geometry
// decision is a pure function in csrc/runtime/launch_geometry.cc. A launch here is three
// steps: knobs(), the planner, the plan copied into CommArgs.
#include "xgmi_comm.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../core/env.h"
#include "../core/trace.h"
#include "xgmi_launch.h"

namespace mxar {

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
  }
}

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static int default_grid(int device) {
  if (const char* g = std::getenv("MXAR_GRID")) return std::max(1, std::atoi(g));
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  return 2 * cus;  // every workgroup must stay resident (they spin): 2 x 256-thread WG per CU
}

int64_t XgmiComm::flag_bytes(int world, int64_t slot_bytes, int threshold_rows, int64_t flag_gran) {
  return mxar::flag_bytes(world, slot_bytes, threshold_rows, flag_gran);
}

XgmiComm::Layout XgmiComm::layout(int world, int64_t slot_bytes, int threshold_rows, int64_t min_flag_bytes,
                                  int64_t flag_gran) {
  int64_t ll_max = 512 * 1024;
  if (const char* e = std::getenv("MXAR_LL_MAX")) ll_max = std::max<int64_t>(0, std::atoll(e));
  return slab_layout(world, slot_bytes, threshold_rows, min_flag_bytes, flag_gran, ll_max);
}

int64_t XgmiComm::ipc_safe_bytes(int64_t bytes) { return mxar::ipc_safe_bytes(bytes); }

XgmiComm::XgmiComm(int rank, int world, int device, int64_t slot_bytes, int grid, double timeout_s,
                   int threshold_rows, char* external_slab, int64_t external_bytes, int64_t min_flag_bytes,
                   uint32_t* external_ctl, int64_t flag_gran)
    : rank_(rank), world_(world), device_(device), grid_(grid), rows_(1 + threshold_rows), timeout_s_(timeout_s) {
  if (threshold_rows < 0 || threshold_rows > 64)
    throw std::invalid_argument("XgmiComm: threshold_rows (maxLag + 1) must be in [0, 64]");
  if (world < 1 || world > kMaxRanks) throw std::invalid_argument("XgmiComm: world must be in [1, 16]");
  if (rank < 0 || rank >= world) throw std::invalid_argument("XgmiComm: bad rank");
  const Layout L = layout(world, slot_bytes, threshold_rows, min_flag_bytes, flag_gran);
  slot_bytes_ = L.slot_bytes;
  maxch_ = L.maxch;
  off_S_ = L.off_S;
  slot_stride_ = L.slot_stride;
  off_R_ = L.off_R;
  off_B_ = 2 * rows_ * world_ * maxch_ * 4;
  ll_max_ = L.ll_max;
  ll_slot_ = L.ll_slot;
  off_LL_ = L.off_LL;
  slab_bytes_ = L.slab_bytes;
  alloc_bytes_ = L.alloc_bytes;
  // Automatic dispatch limits (resolve()), measured with P logical ranks in one launch on one
  // MI355X (bench.py latency_vs_size; round 4, with launch-size grids, profiles/round4/README.md
  // section 9): the low-latency one-shot wins up to 512 KiB at 2 and 4 ranks and 256 KiB at 8
  // (it moves 2x bytes as flag-carrying LL words, so it loses to the plain kernels once they
  // are bandwidth bound: 2 ranks x 1 MiB ll 15.8 vs one-shot 12.1 us); the one-shot (one hop,
  // every rank reads all P inputs) up to 8 MiB at 2 ranks and 2 MiB at 4 (2 x 16 MiB: two-shot
  // 37.4 vs one-shot 42.1 us; 4 x 4 MiB: 32.3 vs 39.4 us); at 8 ranks the two-shot takes over
  // from the low-latency kernel directly. Across GPUs the one-shot reads every peer's whole
  // buffer over its link, so the two-shot's crossover comes no later there.
  // MXAR_LL_AUTO_MAX / MXAR_ONESHOT_MAX override (bytes).
  const int64_t mib = int64_t{1} << 20;
  ll_auto_max_ = world_ <= 4 ? mib / 2 : mib / 4;
  if (const char* e = std::getenv("MXAR_LL_AUTO_MAX")) ll_auto_max_ = std::max<int64_t>(0, std::atoll(e));
  oneshot_max_ = std::min<int64_t>(slot_bytes_, world_ <= 2 ? 8 * mib : world_ <= 4 ? 2 * mib : mib / 4);
  if (const char* e = std::getenv("MXAR_ONESHOT_MAX")) oneshot_max_ = std::min<int64_t>(slot_bytes_, std::atoll(e));
  default_grid_ = default_grid(device);
  if (grid_ <= 0) grid_ = default_grid_;
  if (const char* e = std::getenv("MXAR_SIZE_GRID")) size_grid_ = std::atoi(e) != 0;
  if (const char* f = study_env("MXAR_FENCE")) fence_ = std::atoi(f) & 3;
  // Slab reads are `nt` loads: the acquire after each wait (bit 1) is what orders them after
  // the peers' flags. Without it a stale line could be read, so clearing it is a study-only
  // setting that must be asked for explicitly.
  if (const char* u = study_env("MXAR_TWOSHOT_UNITS")) units_per_wg_ = std::max(1, std::atoi(u));
  if (const char* u = study_env("MXAR_TWOSHOT_SUB")) sub_max_ = std::max(1, std::atoi(u));
  if (const char* d = study_env("MXAR_RING_DEPTH")) ring_depth_ = std::max(1, std::atoi(d));
  if (const char* g = std::getenv("MXAR_RING_GRID")) ring_grid_ = std::max(1, std::atoi(g));
  if (const char* f = study_env("MXAR_RING_FLAGS")) {
    // the round-3 layout whose flag words had two writers (ring hop rows vs other kernels'
    // writer rows): kept only as the negative control of tests/test_comm_gpu.py
    ring_hop_rows_ = std::string(f) == "hop";
  }
  if (const char* g = study_env("MXAR_SLOT_GUARD")) noguard_ = std::atoi(g) == 0;
  // A/B of the threshold kernel's lag-gate shortcut
  if (const char* g = study_env("MXAR_GATE_SHORTCUT")) no_gate_shortcut_ = std::atoi(g) == 0;
  if (const char* g = study_env("MXAR_TH_ONESHOT_MAX")) th_oneshot_max_ = std::max<int64_t>(0, std::atoll(g));
  if (const char* g = study_env("MXAR_TWOSHOT_GEOM")) {
    const std::string v = g;
    geom_ = v == "coarse" ? 0 : v == "fine" ? 1 : v == "flat" ? 2 : -1;
  }
  if (const char* f = study_env("MXAR_TWOSHOT_FLAT_MIN")) flat_min_ = std::max<int64_t>(0, std::atoll(f));

  hip_check(hipSetDevice(device_), "hipSetDevice");
  const char* mem = study_env("MXAR_SLAB_MEM");
  const std::string kind = mem ? mem : "fine";
  // study knobs that trade away correctness guarantees: say so once per communicator
  if (fence_ != 3 || kind != "fine")
    std::fprintf(stderr,
                 "[mxar] WARNING rank %d: study settings active (MXAR_FENCE=%d, MXAR_SLAB_MEM=%s); "
                 "results may be wrong - use the defaults in production\n",
                 rank_, fence_, kind.c_str());
  if (external_slab != nullptr) {
    // An arena owned by the caller (xgmi_plane.cc): allocated fine-grained and zeroed ONCE,
    // exported before any peer knew it, and laid out again on every re-initialisation. Its
    // flags are never zeroed here - a peer may already be writing this epoch's flags; stale
    // flags of an older layout are older epochs, which no wait accepts.
    if (external_bytes < slab_bytes_) throw std::invalid_argument("XgmiComm: external slab too small for the layout");
    slab_ = external_slab;
    own_slab_ = false;
    alloc_bytes_ = external_bytes;
  } else if (kind == "coarse") {
    hip_check(hipMalloc(reinterpret_cast<void**>(&slab_), alloc_bytes_), "hipMalloc(slab)");
  } else {
    const unsigned flags = kind == "fine" ? hipDeviceMallocFinegrained : hipDeviceMallocUncached;
    hip_check(hipExtMallocWithFlags(reinterpret_cast<void**>(&slab_), alloc_bytes_, flags), "hipExtMallocWithFlags(slab)");
  }
  if (own_slab_) {
    // Flags start at 0 = "epoch 0 done"; the first launch uses epoch 1.
    hip_check(hipMemset(slab_, 0, off_S_), "hipMemset(flags)");
    hip_check(hipMemset(slab_ + off_LL_, 0, 2 * world_ * ll_slot_), "hipMemset(ll)");  // epoch 0 never occurs
  }
  if (external_ctl != nullptr && !own_slab_) {
    ctl_ = external_ctl;  // reset by the caller, stream-ordered
    own_ctl_ = false;
  } else {
    hip_check(hipMalloc(reinterpret_cast<void**>(&ctl_), 256), "hipMalloc(ctl)");
    hip_check(hipMemset(ctl_, 0, 256), "hipMemset(ctl)");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  }
  peers_[rank_] = slab_;
}

XgmiComm::~XgmiComm() {
  (void)hipSetDevice(device_);
  if (switch_ev_) (void)hipEventDestroy(switch_ev_);
  for (int k = 0; k < world_; ++k)
    if (ipc_opened_[k] && peers_[k]) (void)hipIpcCloseMemHandle(peers_[k]);
  for (int k = 0; k < static_cast<int>(probe_peers_.size()); ++k)
    if (k != rank_ && probe_peers_[k]) (void)hipIpcCloseMemHandle(probe_peers_[k]);
  if (probe_coarse_) (void)hipFree(probe_coarse_);
  if (sq_part_) (void)hipFree(sq_part_);
  if (slab_ && own_slab_) (void)hipFree(slab_);
  if (ctl_ && own_ctl_) (void)hipFree(ctl_);
}

std::string XgmiComm::ipc_handle() const {
  hipIpcMemHandle_t h;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipIpcGetMemHandle(&h, slab_), "hipIpcGetMemHandle");
  return std::string(reinterpret_cast<const char*>(&h), sizeof(h));
}

void XgmiComm::connect(const std::vector<std::string>& handles) {
  if (static_cast<int>(handles.size()) != world_) throw std::invalid_argument("connect: need one handle per rank");
  hip_check(hipSetDevice(device_), "hipSetDevice");
  for (int k = 0; k < world_; ++k) {
    if (k == rank_) continue;
    if (handles[k].size() != sizeof(hipIpcMemHandle_t)) throw std::invalid_argument("connect: bad handle size");
    hipIpcMemHandle_t h;
    std::memcpy(&h, handles[k].data(), sizeof(h));
    void* p = nullptr;
    static const bool dbg = std::getenv("MXAR_DEBUG_IPC") != nullptr;
    if (dbg) std::fprintf(stderr, "[mxar ipc] rank %d opening rank %d\n", rank_, k);
    hip_check(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
    if (dbg) std::fprintf(stderr, "[mxar ipc] rank %d opened rank %d at %p\n", rank_, k, p);
    peers_[k] = static_cast<char*>(p);
    ipc_opened_[k] = true;
  }
  connected_ = true;
}

void XgmiComm::connect_local(const std::vector<XgmiComm*>& comms) {
  if (static_cast<int>(comms.size()) != world_) throw std::invalid_argument("connect_local: need one comm per rank");
  hip_check(hipSetDevice(device_), "hipSetDevice");
  for (int k = 0; k < world_; ++k) {
    if (comms[k]->slab_bytes_ != slab_bytes_) throw std::invalid_argument("connect_local: slab geometry differs");
    peers_[k] = comms[k]->slab_;
    if (comms[k]->device_ != device_) {
      int can = 0;
      (void)hipDeviceCanAccessPeer(&can, device_, comms[k]->device_);
      if (!can) throw std::runtime_error("connect_local: no peer access between devices");
      hipError_t e = hipDeviceEnablePeerAccess(comms[k]->device_, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) hip_check(e, "hipDeviceEnablePeerAccess");
      (void)hipGetLastError();
    }
  }
  connected_ = true;
}

void XgmiComm::connect_ptrs(const std::vector<char*>& bases) {
  if (static_cast<int>(bases.size()) != world_) throw std::invalid_argument("connect_ptrs: need one base per rank");
  for (int k = 0; k < world_; ++k) {
    if (k == rank_) continue;
    if (bases[k] == nullptr) throw std::invalid_argument("connect_ptrs: null peer slab");
    peers_[k] = bases[k];
  }
  connected_ = true;
}

void XgmiComm::set_grid(int g) { grid_ = g > 0 ? g : default_grid_; }

GridKnobs XgmiComm::knobs() const {
  GridKnobs k;
  k.world = world_;
  k.rows = rows_;
  k.grid = grid_;
  k.default_grid = default_grid_;
  k.size_grid = size_grid_;
  k.maxch = maxch_;
  k.slot_bytes = slot_bytes_;
  k.units_per_wg = units_per_wg_;
  k.sub_max = sub_max_;
  k.geom = geom_;
  k.flat_min = flat_min_;
  k.ring_depth = ring_depth_;
  k.ring_grid = ring_grid_;
  k.th_oneshot_max = th_oneshot_max_;
  k.no_gate_shortcut = no_gate_shortcut_;
  return k;
}

int XgmiComm::shared_launch_cap(int ranks_here) const { return mxar::shared_launch_cap(knobs(), ranks_here); }

int XgmiComm::round_grid(int nch) const { return mxar::round_grid(knobs(), nch); }

static bool capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

void XgmiComm::order_after_last(hipStream_t s) {
  if (launched_ && s != last_stream_) {
    // Graph capture: a captured stream cannot wait on work outside its graph; the caller
    // orders the graph launch (documented in xgmi_comm.h).
    if (!capturing(s) && !capturing(last_stream_)) {
      if (!switch_ev_)
        hip_check(hipEventCreateWithFlags(&switch_ev_, hipEventDisableTiming), "hipEventCreateWithFlags");
      hip_check(hipEventRecord(switch_ev_, last_stream_), "hipEventRecord(stream switch)");
      hip_check(hipStreamWaitEvent(s, switch_ev_, 0), "hipStreamWaitEvent(stream switch)");
      ++stats_.stream_switches;
    }
  }
  launched_ = true;
  last_stream_ = s;
}

void XgmiComm::order_group(const std::vector<XgmiComm*>& group, hipStream_t s) {
  for (XgmiComm* c : group) c->order_after_last(s);
}

std::vector<uint32_t> XgmiComm::ctl_words() const {
  std::vector<uint32_t> w(16, 0);
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipMemcpy(w.data(), ctl_, w.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(ctl)");
  return w;
}

uint32_t XgmiComm::error() const {
  uint32_t e = 0;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipMemcpy(&e, ctl_ + 2, 4, hipMemcpyDeviceToHost), "hipMemcpy(err)");
  return e;
}

void XgmiComm::clear_error() {
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipMemset(ctl_ + 2, 0, 4), "hipMemset(err)");
}

void XgmiComm::reset_local() {
  // Back to the state right after construction: every flag, progress word and LL slot 0
  // (= "epoch 0 done"), epoch / ticket / error / threshold-round counters 0. Only valid when
  // no launch of this communicator is in flight on any rank (XgmiCommunicator.reset
  // brackets it with device synchronisation and host barriers).
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  hip_check(hipMemset(slab_, 0, off_S_), "hipMemset(flags)");
  hip_check(hipMemset(slab_ + off_LL_, 0, 2 * world_ * ll_slot_), "hipMemset(ll)");
  hip_check(hipMemset(ctl_, 0, 256), "hipMemset(ctl)");
  hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
}

void XgmiComm::arm_solo_rehearsal() {
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  hip_check(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(slab_), 0x40000000u, static_cast<size_t>(off_S_ / 4)),
            "hipMemsetD32(flags)");
  // the synthetic peers' contributions in the S / R slots: zeros (the sums stay the input)
  hip_check(hipMemset(slab_ + off_S_, 0, static_cast<size_t>(slab_bytes_ - off_S_)), "hipMemset(slots)");
  hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
}

CommArgs XgmiComm::base_args(const std::vector<XgmiComm*>& group) const {
  CommArgs a;
  std::memset(&a, 0, sizeof(a));
  for (size_t y = 0; y < group.size(); ++y) a.ctl[y] = group[y]->ctl_;
  a.P = world_;
  a.rows = rows_;
  a.rank0 = rank_;
  a.maxch = maxch_;
  a.off_S = off_S_;
  a.off_R = off_R_;
  a.slot_bytes = slot_stride_;
  a.slot_cap = slot_bytes_;
  a.timeout = static_cast<uint64_t>(timeout_s_ * 1e8);
  a.fence = fence_;
  a.rdelay_rank = rdelay_rank_;
  a.rdelay = rdelay_us_ > 0 ? static_cast<uint64_t>(rdelay_us_ * 100.0) : 0;  // 100 MHz ticks
  a.noguard = noguard_ ? 1 : 0;
  for (int k = 0; k < world_; ++k) a.base[k] = peers_[k];
  return a;
}

void XgmiComm::check_group(const std::vector<XgmiComm*>& group, const std::vector<const void*>& ins,
                           const std::vector<void*>& outs, bool need_rows) {
  if (group.empty() || ins.size() != group.size() || outs.size() != group.size())
    throw std::invalid_argument("XgmiComm: one input and one output per rank");
  const XgmiComm& c0 = *group[0];
  for (size_t y = 0; y < group.size(); ++y) {
    const XgmiComm& c = *group[y];
    if (!c.connected_) throw std::runtime_error("XgmiComm: connect() first");
    if (c.device_ != c0.device_ || c.rank_ != c0.rank_ + static_cast<int>(y) || c.world_ != c0.world_ ||
        (need_rows && c.rows_ != c0.rows_))
      throw std::invalid_argument("XgmiComm: a grouped launch needs consecutive ranks on one device");
    if ((reinterpret_cast<uintptr_t>(ins[y]) | reinterpret_cast<uintptr_t>(outs[y])) & 15)
      throw std::invalid_argument("XgmiComm: buffers must be 16-byte aligned");
  }
}

static void set_geometry(CommArgs& a, const LaunchGeometry& g) {
  a.block = g.block;
  a.chunk = g.chunk;
  a.subchunk = g.subchunk;
  a.nch = g.nch;
  a.sub = g.sub;
  a.sgroup = g.sgroup;
}

static void set_adamw_hyper(CommArgs& a, const AdamW& h) {
  a.lr = h.lr;
  a.beta1 = h.beta1;
  a.beta2 = h.beta2;
  a.eps = h.eps;
  a.wd = h.weight_decay;
  adamw_corrections(h.beta1, h.beta2, h.step, &a.c1, &a.c2_sqrt);
}

void adamw_corrections(float beta1, float beta2, int step, float* c1, float* c2_sqrt) {
  *c1 = 1.f - std::pow(beta1, static_cast<float>(step));
  *c2_sqrt = std::sqrt(1.f - std::pow(beta2, static_cast<float>(step)));
}

int adamw_corrections_end(float beta1, float beta2, int cap) {
  auto ones = [&](int t) {
    float c1, c2;
    adamw_corrections(beta1, beta2, t, &c1, &c2);
    return c1 == 1.f && c2 == 1.f;
  };
  if (!ones(cap)) return cap;
  int lo = 0, hi = cap;  // ones(hi), not ones(lo) (count 0 is never applied); beta^t is monotone
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    (ones(mid) ? hi : lo) = mid;
  }
  return hi;
}

void scale_step(int device, const ScaleStepArgs& a, hipStream_t stream) {
  if (a.recs == nullptr || a.state == nullptr || a.rec == nullptr || a.table == nullptr)
    throw std::invalid_argument("scale_step: null buffer");
  if ((reinterpret_cast<uintptr_t>(a.recs) | reinterpret_cast<uintptr_t>(a.state) | reinterpret_cast<uintptr_t>(a.rec)) & 15)
    throw std::invalid_argument("scale_step: records, state and step record must be 16-byte aligned");
  if (a.P < 1 || a.P > kMaxRanks) throw std::invalid_argument("scale_step: world out of range");
  if (a.end < 1 || a.filled < 1 || a.filled > a.end)
    throw std::invalid_argument("scale_step: the correction table needs 1 <= filled <= end");
  if (a.dynamic && a.interval < 1) throw std::invalid_argument("scale_step: growth_interval counts from 1");
  hip_check(hipSetDevice(device), "hipSetDevice");
  launch_scale_step(a, stream);
  hip_check(hipGetLastError(), "scale_step launch");
}

// One launch for the ranks `group` (all on one device, consecutive rank ids starting at
// group[0]->rank()) over one segment of n elements.
void XgmiComm::launch_segment(const std::vector<XgmiComm*>& group, const char* const* ins, char* const* outs,
                              int64_t n, DType dt, hipStream_t stream, Algo kind, float scale) {
  const bool oneshot = kind == Algo::OneShot;
  const bool ring = kind == Algo::Ring || kind == Algo::RingNative;
  const XgmiComm& c0 = *group[0];
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  const int ranks_here = static_cast<int>(group.size());
  const LaunchGeometry g = plan_allreduce(kind, c0.knobs(), n, es, ranks_here);
  CommArgs a = c0.base_args(group);
  for (size_t y = 0; y < group.size(); ++y) {
    a.in[y] = ins[y];
    a.out[y] = outs[y];
  }
  a.n = n;
  set_geometry(a, g);
  a.off_LL = c0.off_LL_;
  a.ll_slot = c0.ll_slot_;
  a.scale = scale;
  a.fdelay_rank = c0.fdelay_rank_;
  a.fdelay = c0.fdelay_us_ > 0 ? static_cast<uint64_t>(c0.fdelay_us_ * 100.0) : 0;
  a.ring_hop_rows = c0.ring_hop_rows_ ? 1 : 0;
  a.stamps = c0.stamps_;
  if (a.stamps != nullptr && g.gx * ranks_here > c0.stamp_slots_) a.stamps = nullptr;  // buffer too small: off
  const dim3 grid(g.gx, ranks_here);
  if (kind == Algo::LL) {
    if (2 * ceil_div(n * es, 8) * 8 > c0.ll_slot_) throw std::logic_error("XgmiComm: LL segment exceeds its slot");
    launch_ll(a, grid, stream, dt);
  } else {
    launch_allreduce(a, grid, stream, dt, kind);
  }
  hip_check(hipGetLastError(), "allreduce launch");
  for (XgmiComm* c : group) {
    ++c->stats_.launches;
    ++(kind == Algo::LL ? c->stats_.ll
                        : oneshot ? c->stats_.oneshot : ring ? c->stats_.ring : c->stats_.twoshot);
  }
}

void XgmiComm::run(const std::vector<XgmiComm*>& group, const std::vector<const void*>& ins,
                   const std::vector<void*>& outs, int64_t n, DType dt, hipStream_t stream, Algo algo, float scale) {
  check_group(group, ins, outs);
  const XgmiComm& c0 = *group[0];
  if (n <= 0) return;
  hip_check(hipSetDevice(c0.device_), "hipSetDevice");
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  for (XgmiComm* c : group) {
    ++c->stats_.calls;
    c->stats_.bytes += n * es;
  }
  order_group(group, stream);
  if (c0.world_ == 1 && scale == 1.f) {  // a 1-rank sum is the identity: copy out-of-place, nothing in place
    for (size_t y = 0; y < group.size(); ++y)
      if (ins[y] != outs[y])
        launch_copy(ins[y], outs[y], n * es, stream);
    return;
  }
  const Algo kind = c0.resolve(n, dt, algo, static_cast<int>(group.size()));
  const bool ll = kind == Algo::LL;
  const bool oneshot = kind == Algo::OneShot;
  TraceScope span("xgmi", [&] {
    return std::make_pair(std::string(ll        ? "ll "
                                      : oneshot ? "oneshot "
                                      : kind == Algo::Ring ? "ring "
                                      : kind == Algo::RingNative ? "ring_native "
                                                           : "twoshot ") +
                              std::to_string(n * es) + "B",
                          "{\"rank\":" + std::to_string(c0.rank_) + ",\"ranks_in_launch\":" +
                              std::to_string(group.size()) + "}");
  });
  // ring: S slots carry fp32 partials, so a block holds slot_bytes / 4 elements
  const int64_t seg = ll ? c0.ll_max_ / es
                      : oneshot ? c0.slot_bytes_ / es
                      : kind == Algo::Ring ? c0.world_ * (c0.slot_bytes_ / 4) : c0.world_ * (c0.slot_bytes_ / es);
  // (RingNative: element-type partials, a block fills a slot like the two-shot's)
  std::vector<const char*> ip(group.size());
  std::vector<char*> op(group.size());
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t len = std::min(seg, n - off);
    for (size_t y = 0; y < group.size(); ++y) {
      ip[y] = static_cast<const char*>(ins[y]) + off * es;
      op[y] = static_cast<char*>(outs[y]) + off * es;
    }
    launch_segment(group, ip.data(), op.data(), len, dt, stream, kind, scale);
  }
}

Algo XgmiComm::resolve(int64_t n, DType dt, Algo algo, int ranks_in_launch) const {
  (void)ranks_in_launch;
  const int64_t bytes = n * static_cast<int64_t>(dtype_size(dt));
  if (algo == Algo::LL) return ll_max_ >= 16 ? Algo::LL : Algo::TwoShot;
  if (algo == Algo::OneShot) return bytes <= slot_bytes_ ? Algo::OneShot : Algo::TwoShot;
  if (algo == Algo::Ring || algo == Algo::RingNative) return algo;
  if (algo == Algo::TwoShot) return Algo::TwoShot;
  // Auto: low-latency one-shot, then one-shot, then two-shot, with size limits per rank count
  // set in the constructor from the bench's latency table (profiles/round3/README.md)
  if (ll_max_ >= 16 && bytes <= ll_auto_max_) return Algo::LL;
  return bytes <= oneshot_max_ ? Algo::OneShot : Algo::TwoShot;
}

int64_t XgmiComm::block_elems(int64_t n, DType dt) const {
  return mxar::block_elems(world_, n, static_cast<int64_t>(dtype_size(dt)));
}

// ---------------------------------------------------------------------------------
// The sharded-data-parallel step: fused (xgmi_adam.hip), or in two launches where a global
// gradient norm is wanted (xgmi_clip.hip) - all three entry points on the `adamw` geometry
// ---------------------------------------------------------------------------------
static bool overlaps(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + static_cast<uintptr_t>(bbytes) && y < x + static_cast<uintptr_t>(abytes);
}

CommArgs XgmiComm::shard_step_args(const std::vector<XgmiComm*>& group, int64_t n, DType dt, const char* what,
                                   hipStream_t stream, dim3* grid) {
  const XgmiComm& c0 = *group[0];
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  for (size_t y = 0; y < group.size(); ++y) {
    const XgmiComm& c = *group[y];
    if (!c.connected_) throw std::runtime_error("XgmiComm: connect() first");
    if (c.device_ != c0.device_ || c.rank_ != c0.rank_ + static_cast<int>(y) || c.world_ != c0.world_)
      throw std::invalid_argument("XgmiComm: a grouped launch needs consecutive ranks on one device");
  }
  if (n * es > c0.world_ * c0.slot_bytes_)
    throw std::invalid_argument(std::string(what) + ": tensor exceeds one launch (n * dtype <= world * slot_bytes)");
  hip_check(hipSetDevice(c0.device_), "hipSetDevice");
  for (XgmiComm* c : group) {
    ++c->stats_.calls;
    c->stats_.bytes += n * es;
  }
  order_group(group, stream);
  const int ranks_here = static_cast<int>(group.size());
  const LaunchGeometry g = plan_allreduce(Algo::TwoShot, c0.knobs(), n, es, ranks_here, true);
  CommArgs a = c0.base_args(group);
  a.n = n;
  set_geometry(a, g);
  *grid = dim3(g.gx, ranks_here);
  return a;
}

void XgmiComm::step_adamw_local(const std::vector<XgmiComm*>& group, const std::vector<const void*>& grads,
                                const std::vector<void*>& params, int64_t n, DType dt, hipStream_t stream,
                                const std::vector<AdamShard>& st, const AdamW& h, float scale) {
  if (group.empty() || grads.size() != group.size() || params.size() != group.size() || st.size() != group.size())
    throw std::invalid_argument("step_adamw: one grads / params / shard state per rank");
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  for (size_t y = 0; y < group.size(); ++y) {
    if ((reinterpret_cast<uintptr_t>(grads[y]) | reinterpret_cast<uintptr_t>(params[y]) |
         reinterpret_cast<uintptr_t>(st[y].param) | reinterpret_cast<uintptr_t>(st[y].exp_avg) |
         reinterpret_cast<uintptr_t>(st[y].exp_avg_sq)) & 15)
      throw std::invalid_argument("step_adamw: buffers must be 16-byte aligned");
    if (overlaps(grads[y], n * es, params[y], n * es))
      throw std::invalid_argument("step_adamw: grads and params must not overlap");
  }
  if (n <= 0) return;
  if (h.step < 1) throw std::invalid_argument("step_adamw: step counts from 1");
  dim3 grid;
  CommArgs a = shard_step_args(group, n, dt, "step_adamw", stream, &grid);
  TraceScope span("xgmi", [&] {
    return std::make_pair("adamw " + std::to_string(n * es) + "B", "{\"rank\":" + std::to_string(group[0]->rank_) + "}");
  });
  for (size_t y = 0; y < group.size(); ++y) {
    a.in[y] = static_cast<const char*>(grads[y]);
    a.out[y] = static_cast<char*>(params[y]);
    a.opt_p[y] = st[y].param;
    a.opt_m[y] = st[y].exp_avg;
    a.opt_v[y] = st[y].exp_avg_sq;
  }
  a.scale = scale;
  set_adamw_hyper(a, h);
  launch_adamw(a, grid, stream, dt);
  hip_check(hipGetLastError(), "adamw launch");
  for (XgmiComm* c : group) {
    ++c->stats_.launches;
    ++c->stats_.adamw;
  }
}

void XgmiComm::step_adamw(const void* grads, void* params, int64_t n, DType dt, hipStream_t stream,
                          const AdamShard& st, const AdamW& h, float scale) {
  step_adamw_local({this}, {grads}, {params}, n, dt, stream, {st}, h, scale);
}

void XgmiComm::reduce_scatter_sq_local(const std::vector<XgmiComm*>& group, const std::vector<const void*>& grads,
                                       const std::vector<float*>& gshards, const std::vector<float*>& sqs, int64_t n,
                                       DType dt, hipStream_t stream, float scale, bool accumulate) {
  if (group.empty() || grads.size() != group.size() || gshards.size() != group.size() || sqs.size() != group.size())
    throw std::invalid_argument("reduce_scatter_sq: one grads / gshard / sq per rank");
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  const int64_t shard_bytes = group[0]->block_elems(n, dt) * 4;
  for (size_t y = 0; y < group.size(); ++y) {
    if ((reinterpret_cast<uintptr_t>(grads[y]) | reinterpret_cast<uintptr_t>(gshards[y])) & 15)
      throw std::invalid_argument("reduce_scatter_sq: buffers must be 16-byte aligned");
    if (sqs[y] == nullptr || (reinterpret_cast<uintptr_t>(sqs[y]) & 3))
      throw std::invalid_argument("reduce_scatter_sq: sq must be a 4-byte aligned fp32");
    if (overlaps(grads[y], n * es, gshards[y], shard_bytes) || overlaps(sqs[y], 4, gshards[y], shard_bytes) ||
        overlaps(sqs[y], 4, grads[y], n * es))
      throw std::invalid_argument("reduce_scatter_sq: grads, gshard and sq must not overlap");
  }
  if (n <= 0) return;
  dim3 grid;
  CommArgs a = shard_step_args(group, n, dt, "reduce_scatter_sq", stream, &grid);
  TraceScope span("xgmi", [&] {
    return std::make_pair(std::string(accumulate ? "rs_sq_acc " : "rs_sq ") + std::to_string(n * es) + "B",
                          "{\"rank\":" + std::to_string(group[0]->rank_) + "}");
  });
  for (size_t y = 0; y < group.size(); ++y) {
    XgmiComm& c = *group[y];
    if (c.sq_part_ == nullptr)  // one partial per reduce unit: nch * sub <= maxch (plan_twoshot)
      hip_check(hipMalloc(&c.sq_part_, static_cast<size_t>(c.maxch_) * sizeof(float)), "hipMalloc(sq partials)");
    a.in[y] = static_cast<const char*>(grads[y]);
    a.gshard[y] = gshards[y];
    a.sq_part[y] = c.sq_part_;
    a.sq_out[y] = sqs[y];
  }
  a.scale = scale;
  launch_rs_sq(a, grid, stream, dt, accumulate);
  hip_check(hipGetLastError(), "rs_sq launch");
  for (XgmiComm* c : group) {
    ++c->stats_.launches;
    ++c->stats_.rs_sq;
    if (accumulate) ++c->stats_.rs_sq_acc;
  }
}

void XgmiComm::reduce_scatter_sq(const void* grads, float* gshard, float* sq, int64_t n, DType dt, hipStream_t stream,
                                 float scale, bool accumulate) {
  reduce_scatter_sq_local({this}, {grads}, {gshard}, {sq}, n, dt, stream, scale, accumulate);
}

void XgmiComm::step_adamw_shard_local(const std::vector<XgmiComm*>& group, const std::vector<const float*>& gshards,
                                      const std::vector<const float*>& coefs, const std::vector<void*>& params,
                                      int64_t n, DType dt, hipStream_t stream, const std::vector<AdamShard>& st,
                                      const AdamW& h, bool record) {
  const int64_t coef_bytes = record ? static_cast<int64_t>(sizeof(StepRecord)) : 4;
  if (group.empty() || gshards.size() != group.size() || coefs.size() != group.size() ||
      params.size() != group.size() || st.size() != group.size())
    throw std::invalid_argument("step_adamw_shard: one gshard / coef / params / shard state per rank");
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  const int64_t shard_bytes = group[0]->block_elems(n, dt) * 4;
  for (size_t y = 0; y < group.size(); ++y) {
    if ((reinterpret_cast<uintptr_t>(gshards[y]) | reinterpret_cast<uintptr_t>(params[y]) |
         reinterpret_cast<uintptr_t>(st[y].param) | reinterpret_cast<uintptr_t>(st[y].exp_avg) |
         reinterpret_cast<uintptr_t>(st[y].exp_avg_sq)) & 15)
      throw std::invalid_argument("step_adamw_shard: buffers must be 16-byte aligned");
    if (coefs[y] == nullptr || (reinterpret_cast<uintptr_t>(coefs[y]) & (record ? 15 : 3)))
      throw std::invalid_argument(record ? "step_adamw_shard: the step record must be 16-byte aligned"
                                         : "step_adamw_shard: coef must be a 4-byte aligned fp32");
    if (overlaps(gshards[y], shard_bytes, params[y], n * es) || overlaps(coefs[y], coef_bytes, params[y], n * es))
      throw std::invalid_argument("step_adamw_shard: gshard, coef and params must not overlap");
    for (const float* s : {st[y].param, st[y].exp_avg, st[y].exp_avg_sq})
      if (overlaps(s, shard_bytes, gshards[y], shard_bytes) || overlaps(s, shard_bytes, coefs[y], coef_bytes))
        throw std::invalid_argument("step_adamw_shard: the shard state must not overlap gshard or coef");
  }
  if (n <= 0) return;
  if (!record && h.step < 1) throw std::invalid_argument("step_adamw_shard: step counts from 1");
  dim3 grid;
  CommArgs a = shard_step_args(group, n, dt, "step_adamw_shard", stream, &grid);
  TraceScope span("xgmi", [&] {
    return std::make_pair("adamw_shard " + std::to_string(n * es) + "B",
                          "{\"rank\":" + std::to_string(group[0]->rank_) + "}");
  });
  for (size_t y = 0; y < group.size(); ++y) {
    a.gshard[y] = const_cast<float*>(gshards[y]);
    a.coef[y] = coefs[y];
    a.out[y] = static_cast<char*>(params[y]);
    a.opt_p[y] = st[y].param;
    a.opt_m[y] = st[y].exp_avg;
    a.opt_v[y] = st[y].exp_avg_sq;
  }
  set_adamw_hyper(a, h);  // record: c1 / c2_sqrt are set and not read
  launch_adamw_shard(a, grid, stream, dt, record);
  hip_check(hipGetLastError(), "adamw_shard launch");
  for (XgmiComm* c : group) {
    ++c->stats_.launches;
    ++c->stats_.adamw_shard;
  }
}

void XgmiComm::step_adamw_shard(const float* gshard, const float* coef, void* params, int64_t n, DType dt,
                                hipStream_t stream, const AdamShard& st, const AdamW& h, bool record) {
  step_adamw_shard_local({this}, {gshard}, {coef}, {params}, n, dt, stream, {st}, h, record);
}

void XgmiComm::allreduce(const void* in, void* out, int64_t n, DType dt, hipStream_t stream, Algo algo, float scale) {
  run({this}, {in}, {out}, n, dt, stream, algo, scale);
}

void XgmiComm::allreduce_local(const std::vector<XgmiComm*>& comms, const std::vector<const void*>& ins,
                               const std::vector<void*>& outs, int64_t n, DType dt, hipStream_t stream, Algo algo,
                               float scale) {
  run(comms, ins, outs, n, dt, stream, algo, scale);
}

int XgmiComm::threshold_chunks(int64_t n, DType dt, int ranks_in_launch) const {
  return plan_threshold(knobs(), n, static_cast<int64_t>(dtype_size(dt)), ranks_in_launch, 1.f, 1.f).nch;
}

bool XgmiComm::threshold_args(const std::vector<XgmiComm*>& group, const std::vector<const void*>& ins,
                              const std::vector<void*>& outs, int64_t n, DType dt, float thr, float thc,
                              int32_t* counts, float scale, bool rescale, const RoundSpec* spec, CommArgs& a,
                              int* gx_out) {
  check_group(group, ins, outs, true);
  const XgmiComm& c0 = *group[0];
  if (c0.rows_ < 2)
    throw std::invalid_argument("allreduce_threshold: construct the comm with threshold_rows = maxLag + 1 >= 1");
  if (!(thr >= 0.f && thr <= 1.f && thc >= 0.f && thc <= 1.f))
    throw std::invalid_argument("allreduce_threshold: thresholds must be in [0, 1]");
  if (n <= 0) return false;
  const int W = c0.world_;
  if (W > 32) throw std::invalid_argument("allreduce_threshold: at most 32 ranks");
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  const int ranks_here = static_cast<int>(group.size());
  RoundShape shape;
  if (spec != nullptr) {
    shape.block = spec->block;
    shape.chunk = spec->chunk;
    shape.order_ref = spec->order_ref;
    shape.split = spec->split_scratch != nullptr && spec->split_bytes >= split_scratch_bytes(W, c0.maxch_);
    shape.lag_skip = spec->lag_wait_us >= 0.0;
  }
  const ThresholdPlan p = plan_threshold(c0.knobs(), n, es, ranks_here, thr, thc, shape);
  a = c0.base_args(group);
  for (size_t y = 0; y < group.size(); ++y) {
    a.in[y] = static_cast<const char*>(ins[y]);
    a.out[y] = static_cast<char*>(outs[y]);
  }
  set_geometry(a, p);
  if (p.split) {
    char* sp = static_cast<char*>(spec->split_scratch);
    a.split_dec = reinterpret_cast<uint64_t*>(sp);
    a.split_ctr = reinterpret_cast<uint32_t*>(sp + static_cast<size_t>(W + 1) * c0.maxch_ * 8);
    a.split_early = reinterpret_cast<uint32_t*>(sp + static_cast<size_t>(W + 1) * c0.maxch_ * 12);
  }
  a.n = n;
  a.trows = c0.rows_ - 1;
  a.scale = scale;
  a.rescale = rescale ? 1 : 0;
  a.min_reduce = p.min_reduce;
  a.min_complete = p.min_complete;
  a.full = p.full;
  a.gate_shortcut = p.gate_shortcut;
  a.oneshot = p.oneshot;
  a.counts = counts;
  if (spec != nullptr) {
    a.epoch_set = spec->epoch;
    a.cold = spec->cold ? 1 : 0;
    a.order_ref = spec->order_ref ? 1 : 0;
    a.hforce = spec->host_force;
    a.habort = spec->host_abort;
    a.err_out = spec->err_out;
    a.done_out = spec->done_out;
    a.counts_host = counts != nullptr ? spec->counts_host : nullptr;
    if (p.lag_skip) {
      a.lag_skip = 1;
      a.lag_wait = static_cast<uint64_t>(spec->lag_wait_us * 100.0);  // s_memrealtime: 100 MHz
    }
  }
  a.delay_rank = -1;
  for (XgmiComm* c : group)
    if (c->delay_rank_ >= 0 && c->delay_us_ > 0) {
      a.delay_rank = c->delay_rank_;
      a.delay = static_cast<uint64_t>(c->delay_us_ * 100.0);  // s_memrealtime: 100 MHz
    }
  a.stamps = c0.stamps_;
  if (a.stamps != nullptr && p.gx * ranks_here > c0.stamp_slots_) a.stamps = nullptr;  // buffer too small: off
  *gx_out = p.gx;
  return true;
}

void XgmiComm::run_threshold(const std::vector<XgmiComm*>& group, const std::vector<const void*>& ins,
                             const std::vector<void*>& outs, int64_t n, DType dt, hipStream_t stream, float thr,
                             float thc, int32_t* counts, float scale, bool rescale, const RoundSpec* spec) {
  CommArgs a;
  int gx = 1;
  if (!threshold_args(group, ins, outs, n, dt, thr, thc, counts, scale, rescale, spec, a, &gx)) return;
  const XgmiComm& c0 = *group[0];
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  const int ranks_here = static_cast<int>(group.size());
  hip_check(hipSetDevice(c0.device_), "hipSetDevice");
  TraceScope span("xgmi", [&] {
    return std::make_pair("threshold " + std::to_string(n * es) + "B",
                          "{\"rank\":" + std::to_string(c0.rank_) + ",\"ranks_in_launch\":" +
                              std::to_string(ranks_here) + "}");
  });
  order_group(group, stream);
  launch_threshold(a, dim3(gx, ranks_here), stream, dt);
  hip_check(hipGetLastError(), "threshold launch");
  for (XgmiComm* c : group) {
    ++c->stats_.calls;
    ++c->stats_.launches;
    ++c->stats_.threshold;
    c->stats_.bytes += n * es;
  }
}

XgmiComm::ResidentPlan XgmiComm::plan_resident(int64_t n, DType dt, float th_reduce, float th_complete,
                                               const RoundSpec& spec, int max_grid, bool allow_split) const {
  ResidentPlan p;
  auto a = std::make_shared<CommArgs>();
  int gx = 0;
  XgmiComm* self = const_cast<XgmiComm*>(this);
  if (!threshold_args({self}, {nullptr}, {nullptr}, n, dt, th_reduce, th_complete, nullptr, 1.f, false, &spec,
                      *a, &gx))
    return p;
  // split chunks (the spec carried split scratch and the geometry used it) run on the launch
  // path of a lone worker; a plane group's kernel runs them
  if ((a->sub > 1 && !allow_split) || gx > max_grid || a->delay_rank >= 0) return p;  // big rounds / test knobs
  p.args = a;
  p.grid = gx;
  p.dt = dt;
  p.n = n;
  return p;
}

void XgmiComm::launch_resident(const ResidentPlan& p, const ResidentDoor* door, uint32_t* hstate, uint32_t* dm,
                               uint32_t seq, uint32_t gen, uint64_t idle_ticks, hipStream_t stream) {
  if (!p.args || p.grid <= 0) throw std::invalid_argument("launch_resident: no resident plan");
  hip_check(hipSetDevice(device_), "hipSetDevice");
  order_after_last(stream);
  launch_threshold_resident(*p.args, p.grid, stream, p.dt, door, hstate, dm, seq, gen, idle_ticks);
  hip_check(hipGetLastError(), "resident threshold launch");
  ++stats_.launches;
}

void XgmiComm::publish_progress(uint32_t value, hipStream_t stream) {
  if (!connected_) throw std::runtime_error("XgmiComm: connect() first");
  if (rows_ < 2) throw std::invalid_argument("publish_progress: no threshold rows");
  hip_check(hipSetDevice(device_), "hipSetDevice");
  order_after_last(stream);
  launch_publish_progress(base_args({}), value, stream);
  hip_check(hipGetLastError(), "publish_progress launch");
}

void XgmiComm::round(const void* in, void* out, int64_t n, DType dt, hipStream_t stream, float th_reduce,
                     float th_complete, int32_t* counts, const RoundSpec& spec, float scale) {
  run_threshold({this}, {in}, {out}, n, dt, stream, th_reduce, th_complete, counts, scale, false, &spec);
}

// Two rounds of co-located workers may share a launch: the same geometry, thresholds and slabs.
static bool same_round_shape(const CommArgs& b, const CommArgs& a0) {
  bool same = b.n == a0.n && b.block == a0.block && b.chunk == a0.chunk && b.subchunk == a0.subchunk &&
              b.nch == a0.nch && b.sub == a0.sub && b.sgroup == a0.sgroup && b.P == a0.P && b.rows == a0.rows &&
              b.full == a0.full && b.min_reduce == a0.min_reduce &&
              b.min_complete == a0.min_complete && b.maxch == a0.maxch && b.off_S == a0.off_S && b.off_R == a0.off_R &&
              b.slot_bytes == a0.slot_bytes && b.order_ref == a0.order_ref && b.fence == a0.fence &&
              b.gate_shortcut == a0.gate_shortcut && b.scale == a0.scale && b.rescale == a0.rescale &&
              b.timeout == a0.timeout;
  for (int k = 0; same && k < a0.P; ++k) same = b.base[k] == a0.base[k];
  return same;
}

void XgmiComm::launch_group_resident(const std::vector<XgmiComm*>& comms, const std::vector<const ResidentPlan*>& plans,
                                     const std::vector<GroupResidentMember>& members, uint32_t* gstate, uint64_t* gdm,
                                     uint32_t gen, uint64_t idle_ticks, hipStream_t stream) {
  const int Y = static_cast<int>(plans.size());
  if (Y < 1 || Y > kMaxRanks || comms.size() != plans.size() || members.size() != plans.size())
    throw std::invalid_argument("launch_group_resident: one communicator, plan and member per worker, at most " +
                                std::to_string(kMaxRanks));
  for (const ResidentPlan* p : plans)
    if (p == nullptr || !p->args || p->grid <= 0) throw std::invalid_argument("launch_group_resident: no resident plan");
  const ResidentPlan& p0 = *plans[0];
  const CommArgs& a0 = *p0.args;
  CommArgs a = a0;
  GroupResArgs g;
  std::memset(&g, 0, sizeof(g));
  for (int y = 0; y < Y; ++y) {
    const ResidentPlan& p = *plans[y];
    const CommArgs& b = *p.args;
    if (p.grid != p0.grid || p.dt != p0.dt || p.n != p0.n || comms[y]->device_ != comms[0]->device_ ||
        !same_round_shape(b, a0))
      throw std::invalid_argument("launch_group_resident: the workers' rounds must share geometry and slabs");
    a.ctl[y] = comms[y]->ctl_;
    g.m[y] = members[y];
    g.m[y].rank = comms[y]->rank_;
    g.m[y].stamps = comms[y]->stamp_slots_ >= p0.grid ? comms[y]->stamps_ : nullptr;  // study knob
    g.m[y].split_dec = b.split_dec;  // each worker's own scratch (its plan's spec)
    g.m[y].split_ctr = b.split_ctr;
    g.m[y].split_early = b.split_early;
  }
  a.stamps = nullptr;
  a.delay_rank = -1;
  g.gstate = gstate;
  g.gdm = gdm;
  g.idle = idle_ticks;
  g.gen = gen;
  g.Y = Y;
  hip_check(hipSetDevice(comms[0]->device_), "hipSetDevice");
  order_group(comms, stream);
  launch_threshold_group_resident(a, g, p0.grid, stream, p0.dt);
  hip_check(hipGetLastError(), "group resident threshold launch");
  for (XgmiComm* c : comms) ++c->stats_.launches;
}

void XgmiComm::allreduce_threshold(const void* in, void* out, int64_t n, DType dt, hipStream_t stream,
                                   float th_reduce, float th_complete, int32_t* counts, float scale, bool rescale) {
  run_threshold({this}, {in}, {out}, n, dt, stream, th_reduce, th_complete, counts, scale, rescale);
}

void XgmiComm::allreduce_threshold_local(const std::vector<XgmiComm*>& comms, const std::vector<const void*>& ins,
                                         const std::vector<void*>& outs, int64_t n, DType dt, hipStream_t stream,
                                         float th_reduce, float th_complete, int32_t* counts, float scale,
                                         bool rescale) {
  run_threshold(comms, ins, outs, n, dt, stream, th_reduce, th_complete, counts, scale, rescale);
}

void XgmiComm::barrier_group(const std::vector<XgmiComm*>& group, hipStream_t stream) {
  const XgmiComm& c0 = *group[0];
  for (XgmiComm* c : group)
    if (!c->connected_) throw std::runtime_error("XgmiComm: connect() first");
  hip_check(hipSetDevice(c0.device_), "hipSetDevice");
  CommArgs a = c0.base_args(group);
  a.fence = 3;
  order_group(group, stream);
  launch_barrier(a, dim3(1, static_cast<unsigned>(group.size())), stream);
  hip_check(hipGetLastError(), "barrier launch");
}

void XgmiComm::barrier(hipStream_t stream) { barrier_group({this}, stream); }

void XgmiComm::run_coll(const std::vector<XgmiComm*>& group, Coll op, const std::vector<const void*>& ins,
                        const std::vector<void*>& outs, int64_t m, DType dt, hipStream_t stream, float scale) {
  check_group(group, ins, outs);
  const XgmiComm& c0 = *group[0];
  const int W = c0.world_;
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  const int64_t in_blocks = op == Coll::AllGather ? 1 : W, out_blocks = op == Coll::ReduceScatter ? 1 : W;
  for (size_t y = 0; y < group.size(); ++y) {
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(ins[y]), o0 = reinterpret_cast<uintptr_t>(outs[y]);
    if (i0 < o0 + static_cast<uintptr_t>(out_blocks * m * es) && o0 < i0 + static_cast<uintptr_t>(in_blocks * m * es))
      throw std::invalid_argument("XgmiComm: collective input and output must not overlap");
  }
  if ((m * es) & 15) throw std::invalid_argument("XgmiComm: block size (m x dtype) must be a multiple of 16 bytes");
  if (m <= 0) return;
  hip_check(hipSetDevice(c0.device_), "hipSetDevice");
  for (XgmiComm* c : group) {
    ++c->stats_.calls;
    c->stats_.bytes += in_blocks * m * es;
  }
  order_group(group, stream);
  if (W == 1) {  // one rank: a copy (scaled for reduce-scatter)
    for (size_t y = 0; y < group.size(); ++y) {
      if (op == Coll::ReduceScatter && scale != 1.f)
        launch_reduce_slots(ins[y], m, 1, outs[y], m, dt, scale, stream);
      else
        launch_copy(ins[y], outs[y], m * es, stream);
    }
    return;
  }
  static const char* names[] = {"all_to_all ", "all_gather ", "reduce_scatter "};
  TraceScope span("xgmi", [&] {
    return std::make_pair(std::string(names[static_cast<int>(op)]) + std::to_string(in_blocks * m * es) + "B",
                          "{\"rank\":" + std::to_string(c0.rank_) + ",\"ranks_in_launch\":" +
                              std::to_string(group.size()) + "}");
  });
  const int ranks_here = static_cast<int>(group.size());
  const GridKnobs knobs = c0.knobs();
  const int64_t seg = c0.slot_bytes_ / es;  // per block per launch
  for (int64_t off = 0; off < m; off += seg) {
    const int64_t len = std::min(seg, m - off);
    const LaunchGeometry g = plan_coll(op, knobs, len, es, ranks_here);
    CommArgs a = c0.base_args(group);
    for (size_t y = 0; y < group.size(); ++y) {
      a.in[y] = static_cast<const char*>(ins[y]) + off * es;
      a.out[y] = static_cast<char*>(outs[y]) + off * es;
    }
    set_geometry(a, g);
    a.n = len;
    a.block = m;
    a.scale = scale;
    launch_coll(a, dim3(g.gx, ranks_here), stream, dt, static_cast<int>(op));
    hip_check(hipGetLastError(), "collective launch");
    for (XgmiComm* c : group) {
      ++c->stats_.launches;
      ++c->stats_.coll;
    }
  }
}

void XgmiComm::collective(Coll op, const void* in, void* out, int64_t m, DType dt, hipStream_t stream, float scale) {
  run_coll({this}, op, {in}, {out}, m, dt, stream, scale);
}

void XgmiComm::collective_local(const std::vector<XgmiComm*>& comms, Coll op, const std::vector<const void*>& ins,
                                const std::vector<void*>& outs, int64_t m, DType dt, hipStream_t stream,
                                float scale) {
  run_coll(comms, op, ins, outs, m, dt, stream, scale);
}

void XgmiComm::run_rooted(const std::vector<XgmiComm*>& group, Rooted kind, const std::vector<const void*>& ins,
                          const std::vector<void*>& outs_in, int64_t n, DType dt, int root, hipStream_t stream,
                          float scale) {
  const bool reduce = kind == Rooted::Reduce;
  std::vector<void*> outs = outs_in;
  if (reduce && !group.empty() && outs.size() == group.size())
    for (size_t y = 0; y < group.size(); ++y)
      if (group[y]->rank_ != root) outs[y] = nullptr;  // ignored off the root
  check_group(group, ins, outs);
  const XgmiComm& c0 = *group[0];
  const int W = c0.world_;
  if (root < 0 || root >= W) throw std::invalid_argument("XgmiComm: root must be in [0, world)");
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  if (reduce && n > 0)
    for (size_t y = 0; y < group.size(); ++y) {
      if (group[y]->rank_ != root) continue;
      if (outs[y] == nullptr) throw std::invalid_argument("XgmiComm: reduce needs an output on the root");
      const uintptr_t i0 = reinterpret_cast<uintptr_t>(ins[y]), o0 = reinterpret_cast<uintptr_t>(outs[y]);
      if (i0 < o0 + static_cast<uintptr_t>(n * es) && o0 < i0 + static_cast<uintptr_t>(n * es))
        throw std::invalid_argument("XgmiComm: reduce input and output must not overlap on the root");
    }
  if (n <= 0) return;
  hip_check(hipSetDevice(c0.device_), "hipSetDevice");
  for (XgmiComm* c : group) {
    ++c->stats_.calls;
    c->stats_.bytes += n * es;
  }
  order_group(group, stream);
  if (W == 1) {  // one rank: nothing to send; a reduce is a copy (scaled)
    for (size_t y = 0; reduce && y < group.size(); ++y) {
      if (scale != 1.f)
        launch_reduce_slots(ins[y], 0, 1, outs[y], n, dt, scale, stream);  // one slot: no stride (any n)
      else
        launch_copy(ins[y], outs[y], n * es, stream);
    }
    return;
  }
  TraceScope span("xgmi", [&] {
    return std::make_pair(std::string(reduce ? "reduce " : "broadcast ") + std::to_string(n * es) + "B",
                          "{\"rank\":" + std::to_string(c0.rank_) + ",\"root\":" + std::to_string(root) +
                              ",\"ranks_in_launch\":" + std::to_string(group.size()) + "}");
  });
  const int ranks_here = static_cast<int>(group.size());
  const GridKnobs knobs = c0.knobs();
  const int64_t seg = W * (c0.slot_bytes_ / es);  // one block fits one slot, as the two-shot's segments
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t len = std::min(seg, n - off);
    const LaunchGeometry g = plan_rooted(kind, knobs, len, es, ranks_here);
    CommArgs a = c0.base_args(group);
    for (size_t y = 0; y < group.size(); ++y) {
      a.in[y] = static_cast<const char*>(ins[y]) + off * es;
      a.out[y] = outs[y] == nullptr ? nullptr : static_cast<char*>(outs[y]) + off * es;
    }
    set_geometry(a, g);
    a.n = len;
    a.scale = scale;
    a.root = root;
    launch_rooted(a, dim3(g.gx, ranks_here), stream, dt, kind);
    hip_check(hipGetLastError(), "rooted collective launch");
    for (XgmiComm* c : group) {
      ++c->stats_.launches;
      ++c->stats_.coll;
    }
  }
}

void XgmiComm::broadcast(void* buf, int64_t n, DType dt, int root, hipStream_t stream) {
  run_rooted({this}, Rooted::Broadcast, {buf}, {buf}, n, dt, root, stream, 1.f);
}

void XgmiComm::reduce(const void* in, void* out, int64_t n, DType dt, int root, hipStream_t stream, float scale) {
  run_rooted({this}, Rooted::Reduce, {in}, {out}, n, dt, root, stream, scale);
}

void XgmiComm::broadcast_local(const std::vector<XgmiComm*>& comms, const std::vector<void*>& bufs, int64_t n,
                               DType dt, int root, hipStream_t stream) {
  run_rooted(comms, Rooted::Broadcast, std::vector<const void*>(bufs.begin(), bufs.end()), bufs, n, dt, root, stream,
             1.f);
}

void XgmiComm::reduce_local(const std::vector<XgmiComm*>& comms, const std::vector<const void*>& ins,
                            const std::vector<void*>& outs, int64_t n, DType dt, int root, hipStream_t stream,
                            float scale) {
  run_rooted(comms, Rooted::Reduce, ins, outs, n, dt, root, stream, scale);
}


}  // namespace mxar
