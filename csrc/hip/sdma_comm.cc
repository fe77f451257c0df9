// SdmaComm, host side (sdma_comm.h): HSA agents and engines, the per-call signal ring and the
// SDMA submissions. Every shape decision - segment, pieces, 4 KiB parts, arm values, the order
// of the copies, the slab map - is a pure function in csrc/runtime/sdma_schedule.cc; the
// kernels and their launchers live in sdma_comm.hip (sdma_launch.h).
#include "sdma_comm.h"

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

#include "sdma_launch.h"

namespace mxar {

namespace {

void hsa_check(hsa_status_t s, const char* what) {
  if (s != HSA_STATUS_SUCCESS) {
    const char* m = nullptr;
    hsa_status_string(s, &m);
    throw std::runtime_error(std::string("HSA error in ") + what + ": " + (m ? m : "?"));
  }
}

// The HSA agent at a PCI location ((domain << 32) | bdf; 0 handle: none) and the first CPU agent.
struct Agents {
  uint64_t want = 0;
  hsa_agent_t found{0};
  hsa_agent_t cpu{0};
};

hsa_status_t agent_cb(hsa_agent_t a, void* data) {
  auto* s = static_cast<Agents*>(data);
  hsa_device_type_t t;
  hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t);
  if (t == HSA_DEVICE_TYPE_CPU && s->cpu.handle == 0) s->cpu = a;
  if (t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
  uint32_t bdf = 0, dom = 0;
  hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_BDFID), &bdf);
  hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_DOMAIN), &dom);
  const uint64_t loc = (static_cast<uint64_t>(dom) << 32) | (bdf & ~0x7u);
  if (loc == s->want) s->found = a;
  return HSA_STATUS_SUCCESS;
}

Agents find_agents(uint64_t pci_location) {
  Agents s;
  s.want = pci_location;
  hsa_check(hsa_iterate_agents(agent_cb, &s), "hsa_iterate_agents");
  return s;
}

// The engines towards `dst` from `src`, first answer per (dst, src) kept for the process.
uint32_t cached_engine_status(hsa_agent_t dst, hsa_agent_t src) {
  static std::mutex mu;
  static std::map<std::pair<uint64_t, uint64_t>, uint32_t> seen;
  std::lock_guard<std::mutex> g(mu);
  const auto key = std::make_pair(dst.handle, src.handle);
  auto it = seen.find(key);
  if (it != seen.end()) return it->second;
  uint32_t m = 0;
  if (hsa_amd_memory_copy_engine_status(dst, src, &m) != HSA_STATUS_SUCCESS) m = 0;
  seen[key] = m;
  return m;
}

// The device's SDMA engines. The ROCm 7.0 runtime torch ships answers the same-agent query
// with HSA_STATUS_ERROR_INVALID_AGENT (7.2 answers it); the host <-> device directions name
// the same engines there. The first answer per (dst, src) agent pair is kept for the
// process, so every communicator of it picks its engines from the same mask.
uint32_t engine_mask(hsa_agent_t own, hsa_agent_t cpu) {
  uint32_t mask = cached_engine_status(own, own);
  if (mask == 0 && cpu.handle != 0) mask = cached_engine_status(own, cpu) | cached_engine_status(cpu, own);
  return mask;
}

std::vector<hsa_amd_sdma_engine_id_t> pick_engines(hsa_agent_t dst, hsa_agent_t src, int k, int epp, uint32_t allowed) {
  std::vector<hsa_amd_sdma_engine_id_t> out;
  for (uint32_t e : sdma_pick_engines(cached_engine_status(dst, src), allowed, k, epp))
    out.push_back(static_cast<hsa_amd_sdma_engine_id_t>(e));
  return out;
}

// Owners: what a constructor took is released when it throws, too.
struct HsaRef {
  bool up = false;
  void init() {
    hsa_check(hsa_init(), "hsa_init");
    up = true;
  }
  ~HsaRef() {
    if (up) hsa_shut_down();
  }
};
template <class T>
struct DeviceMem {
  T* p = nullptr;
  ~DeviceMem() {
    if (p) (void)hipFree(p);
  }
};
struct Signal {
  hsa_signal_t s{0};
  Signal() = default;
  Signal(Signal&& o) noexcept : s(o.s) { o.s.handle = 0; }
  Signal(const Signal&) = delete;
  ~Signal() {
    if (s.handle) hsa_signal_destroy(s);
  }
  // the address of the signal's value: what a kernel stores to
  int64_t* value_pointer(const char* what) const {
    volatile hsa_signal_value_t* p = nullptr;
    hsa_check(hsa_amd_signal_value_pointer(s, &p), what);
    return const_cast<int64_t*>(reinterpret_cast<volatile int64_t*>(p));
  }
};

}  // namespace

uint64_t pci_location(int device) {
  int bus = 0, dev = 0, dom = 0;
  (void)hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device);
  (void)hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, device);
  (void)hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device);
  return (static_cast<uint64_t>(dom) << 32) | static_cast<uint64_t>((bus << 8) | (dev << 3));
}

// Engine copies of `bytes` from src to dst on this device, split over `nengines` engines
// (from index `engine` of the device's mask) running at once, `iters` times back to back;
// ms per copy by the host clock. The probe behind profiles/round6 section 3 (which
// buffers, and how many engines at once, the engines are slow on).
double sdma_copy_probe(int device, uint64_t dst, uint64_t src, int64_t bytes, int engine, int iters, int nengines) {
  hip_check(hipSetDevice(device), "hipSetDevice");
  hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  hsa_check(hsa_init(), "hsa_init");
  const Agents s = find_agents(pci_location(device));
  if (s.found.handle == 0) throw std::runtime_error("sdma_copy_probe: no HSA agent for the device");
  const std::vector<uint32_t> engines = sdma_engine_ids(engine_mask(s.found, s.cpu));
  if (engines.empty()) throw std::runtime_error("sdma_copy_probe: no SDMA engine");
  const SdmaParts parts = sdma_parts(bytes, std::max(1, nengines));
  hsa_signal_t done;
  hsa_check(hsa_signal_create(1, 0, nullptr, &done), "signal");
  auto one = [&] {
    hsa_signal_store_relaxed(done, parts.count);
    for (int e = 0; e < parts.count; ++e) {
      const auto eng = static_cast<hsa_amd_sdma_engine_id_t>(engines[static_cast<size_t>(engine + e) % engines.size()]);
      hsa_check(hsa_amd_memory_async_copy_on_engine(reinterpret_cast<void*>(dst + parts.off(e)), s.found,
                                                    reinterpret_cast<const void*>(src + parts.off(e)), s.found,
                                                    static_cast<size_t>(parts.len(e)), 0, nullptr, done, eng, true),
                "hsa_amd_memory_async_copy_on_engine");
    }
    if (hsa_signal_wait_scacquire(done, HSA_SIGNAL_CONDITION_EQ, 0, 10'000'000'000ull, HSA_WAIT_STATE_ACTIVE) != 0)
      throw std::runtime_error("sdma_copy_probe: copy did not complete");
  };
  one();  // warm
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) one();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / iters;
  hsa_signal_destroy(done);
  hsa_shut_down();
  return ms;
}

std::string sdma_diagnose(int device) {
  std::string out;
  hip_check(hipSetDevice(device), "hipSetDevice");
  hsa_status_t st = hsa_init();
  out += "hsa_init=" + std::to_string(static_cast<int>(st));
  const uint64_t want = pci_location(device);
  out += " want=" + std::to_string(want);
  struct Ctx {
    std::string* out;
    hsa_agent_t cpu;
  } ctx{&out, hsa_agent_t{0}};
  if (st == HSA_STATUS_SUCCESS) ctx.cpu = find_agents(want).cpu;
  hsa_iterate_agents(
      [](hsa_agent_t a, void* d) -> hsa_status_t {
        auto* c = static_cast<Ctx*>(d);
        hsa_device_type_t t;
        hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t);
        uint32_t bdf = 0, dom = 0, mask = 0;
        hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_BDFID), &bdf);
        hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_DOMAIN), &dom);
        hsa_status_t s = HSA_STATUS_SUCCESS;
        uint32_t m2 = 0;
        if (t == HSA_DEVICE_TYPE_GPU) s = hsa_amd_memory_copy_engine_status(a, a, &mask);
        *c->out += " | gpu<-gpu status=" + std::to_string(static_cast<int>(s)) + " mask=" + std::to_string(mask);
        if (t == HSA_DEVICE_TYPE_GPU) {
          s = hsa_amd_memory_copy_engine_status(a, c->cpu, &m2);
          *c->out += " gpu<-cpu status=" + std::to_string(static_cast<int>(s)) + " mask=" + std::to_string(m2);
          s = hsa_amd_memory_copy_engine_status(c->cpu, a, &m2);
          *c->out += " cpu<-gpu status=" + std::to_string(static_cast<int>(s)) + " mask=" + std::to_string(m2);
        }
        *c->out += " | agent type=" + std::to_string(static_cast<int>(t)) + " bdf=" + std::to_string(bdf) +
                   " dom=" + std::to_string(dom) + " status=" + std::to_string(static_cast<int>(s)) +
                   " mask=" + std::to_string(mask);
        return HSA_STATUS_SUCCESS;
      },
      &ctx);
  if (st == HSA_STATUS_SUCCESS) hsa_shut_down();
  return out;
}

// Members in the order they are taken; released in reverse.
struct SdmaComm::Impl {
  HsaRef hsa;
  hsa_agent_t own{0}, cpu{0};
  std::vector<hsa_agent_t> peer_agent;
  std::vector<std::vector<hsa_amd_sdma_engine_id_t>> peer_engines;  // engines towards peer k
  DeviceMem<char> slab;
  DeviceMem<uint32_t> err;  // device error word
  DeviceMem<uint32_t> cnt;  // device: per-piece workgroup tickets of the reduce kernel
  struct Pinned {
    uint32_t* p = nullptr;  // epoch words, one per slot (the flag copies' source)
    ~Pinned() {
      if (p) (void)hipHostFree(p);
    }
  } words;
  struct Event {
    hipEvent_t e = nullptr;
    ~Event() {
      if (e) (void)hipEventDestroy(e);
    }
  } sysrel;
  struct Slot {
    Signal start, scf, gdf;
    Signal mid[kSdmaMaxPieces];
    int64_t* start_p = nullptr;
    int64_t* mid_p[kSdmaMaxPieces]{};
    // completion of a piece's data parts: phase 1 per peer ([j * K + k]), phase 2 over every
    // peer ([k]: the own FR flag needs them all, and a copy with one dependency is the form the
    // engines are known to take), armed to the part count - every part's completion
    // decrements it, the piece's flag copies wait for 0. Memory-only signals (the host never
    // waits on them, so no interrupt events - KFD has few), grown on demand.
    std::vector<Signal> c1, c2;
    bool used = false;
    hsa_signal_t of(SdmaSigRef r) const {
      switch (r.kind) {
        case SdmaSig::Start: return start.s;
        case SdmaSig::Mid: return mid[r.index].s;
        case SdmaSig::C1: return c1[static_cast<size_t>(r.index)].s;
        case SdmaSig::C2: return c2[static_cast<size_t>(r.index)].s;
        case SdmaSig::Scf: return scf.s;
        default: return gdf.s;
      }
    }
  };
  static void grow(std::vector<Signal>& v, size_t need) {
    while (v.size() < need) {
      Signal x;
      hsa_check(hsa_amd_signal_create(0, 0, nullptr, HSA_AMD_SIGNAL_AMD_GPU_ONLY, &x.s), "signal(piece)");
      v.push_back(std::move(x));
    }
  }
  Slot slots[kSdmaSlots];
  SdmaSchedule sched;  // scratch of plan(): no allocation per call
};

SdmaComm::SdmaComm(int rank, int world, int device, int64_t slot_bytes, int grid, int engines_per_peer,
                   double timeout_s)
    : rank_(rank), world_(world), device_(device), slot_bytes_(sdma_slot_bytes(slot_bytes)),
      grid_(std::max(1, grid)), epp_(std::max(0, engines_per_peer)), timeout_s_(timeout_s),
      impl_(std::make_unique<Impl>()) {
  if (world < 1 || world > kSdmaMaxWorld || rank < 0 || rank >= world)
    throw std::invalid_argument("SdmaComm: bad rank / world");
  Impl& m = *impl_;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  m.hsa.init();
  const Agents s = find_agents(pci_location(device_));
  if (s.found.handle == 0) throw std::runtime_error("SdmaComm: no HSA agent at the HIP device's PCI location");
  m.own = s.found;
  m.cpu = s.cpu;
  engines_ = engine_mask(m.own, m.cpu);
  if (engines_ == 0) throw std::runtime_error("SdmaComm: the device reports no SDMA engine");

  slab_bytes_ = sdma_slab_bytes(world_, slot_bytes_);
  hip_check(hipExtMallocWithFlags(reinterpret_cast<void**>(&m.slab.p), slab_bytes_, hipDeviceMallocFinegrained),
            "hipExtMallocWithFlags(sdma slab)");
  hip_check(hipMemset(m.slab.p, 0, kFlagBytes), "hipMemset(sdma flags)");
  hip_check(hipMalloc(reinterpret_cast<void**>(&m.err.p), 64), "hipMalloc(err)");
  hip_check(hipMemset(m.err.p, 0, 64), "hipMemset(err)");
  hip_check(hipHostMalloc(reinterpret_cast<void**>(&m.words.p), kSdmaSlots * 64, hipHostMallocCoherent),
            "hipHostMalloc(epoch words)");
  std::memset(m.words.p, 0, kSdmaSlots * 64);
  hip_check(hipEventCreateWithFlags(&m.sysrel.e, hipEventDisableTiming | hipEventReleaseToSystem),
            "hipEventCreate(release to system)");
  hip_check(hipMalloc(reinterpret_cast<void**>(&m.cnt.p), kSdmaMaxPieces * 4), "hipMalloc(piece tickets)");
  hip_check(hipMemset(m.cnt.p, 0, kSdmaMaxPieces * 4), "hipMemset(piece tickets)");
  for (auto& sl : m.slots) {
    hsa_check(hsa_amd_signal_create(1, 0, nullptr, HSA_AMD_SIGNAL_IPC, &sl.start.s), "signal(start)");
    sl.start_p = sl.start.value_pointer("signal_value_pointer(start)");
    for (int k = 0; k < kSdmaMaxPieces; ++k) {
      hsa_check(hsa_amd_signal_create(1, 0, nullptr, HSA_AMD_SIGNAL_IPC, &sl.mid[k].s), "signal(mid)");
      sl.mid_p[k] = sl.mid[k].value_pointer("signal_value_pointer(mid)");
    }
    for (Signal* x : {&sl.scf, &sl.gdf}) hsa_check(hsa_signal_create(0, 0, nullptr, &x->s), "signal");
  }
  hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  peers_.assign(world_, nullptr);
  opened_.assign(world_, false);
  peers_[rank_] = m.slab.p;
}

SdmaComm::~SdmaComm() {
  (void)hipSetDevice(device_);
  (void)hipDeviceSynchronize();
  // no copy of ours may still target a peer slab we are about to unmap
  // (every data part precedes a flag copy counted in scf / gdf)
  for (auto& sl : impl_->slots)
    for (hsa_signal_t x : {sl.scf.s, sl.gdf.s})
      if (x.handle) (void)hsa_signal_wait_scacquire(x, HSA_SIGNAL_CONDITION_EQ, 0, 2000000000ull, HSA_WAIT_STATE_BLOCKED);
  for (int k = 0; k < world_; ++k)
    if (opened_[k] && peers_[k]) (void)hipIpcCloseMemHandle(peers_[k]);
}

std::string SdmaComm::handle() const {
  hipIpcMemHandle_t h;
  hip_check(hipIpcGetMemHandle(&h, impl_->slab.p), "hipIpcGetMemHandle(sdma slab)");
  const uint64_t loc = pci_location(device_);
  std::string out(reinterpret_cast<const char*>(&h), sizeof(h));
  out.append(reinterpret_cast<const char*>(&loc), sizeof(loc));
  return out;
}

int SdmaComm::engines() const { return static_cast<int>(sdma_engine_ids(engines_).size()); }

void SdmaComm::connect(const std::vector<std::string>& handles) {
  if (static_cast<int>(handles.size()) != world_) throw std::invalid_argument("SdmaComm.connect: one handle per rank");
  impl_->peer_agent.assign(world_, impl_->own);
  impl_->peer_engines.assign(world_, {});
  if (epp_ == 0) epp_ = sdma_auto_epp(engines(), world_);
  hip_check(hipSetDevice(device_), "hipSetDevice");
  for (int k = 0; k < world_; ++k) {
    if (k == rank_) continue;
    const std::string& h = handles[k];
    if (h.size() != sizeof(hipIpcMemHandle_t) + 8) throw std::invalid_argument("SdmaComm.connect: bad handle");
    hipIpcMemHandle_t ih;
    std::memcpy(&ih, h.data(), sizeof(ih));
    uint64_t loc = 0;
    std::memcpy(&loc, h.data() + sizeof(ih), 8);
    void* p = nullptr;
    hip_check(hipIpcOpenMemHandle(&p, ih, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle(sdma slab)");
    peers_[k] = static_cast<char*>(p);
    opened_[k] = true;
    const Agents s = find_agents(loc);
    if (s.found.handle != 0) impl_->peer_agent[k] = s.found;
    impl_->peer_engines[k] = pick_engines(impl_->peer_agent[k], impl_->own, k, epp_, engines_);
  }
  connected_ = true;
}

void SdmaComm::connect_local(const std::vector<SdmaComm*>& comms) {
  if (static_cast<int>(comms.size()) != world_) throw std::invalid_argument("SdmaComm.connect_local: one comm per rank");
  // Ranks of one process share its SDMA queues (one per engine): a rank's phase-2 copies
  // wait in an engine queue for its own reduce, which needs the peers' phase-1 copies - so
  // each local rank gets engines of its own (no copy of a peer ever queues behind them).
  const uint32_t mine = sdma_engine_share(engines_, world_, rank_);
  if (mine == 0) throw std::runtime_error("SdmaComm.connect_local: fewer SDMA engines than local ranks");
  engines_ = mine;
  if (epp_ == 0) epp_ = sdma_auto_epp(engines(), world_);
  impl_->peer_agent.assign(world_, impl_->own);
  impl_->peer_engines.assign(world_, {});
  for (int k = 0; k < world_; ++k) {
    if (comms[k]->slot_bytes_ != slot_bytes_ || comms[k]->device_ != device_)
      throw std::invalid_argument("SdmaComm.connect_local: slab geometry / device differs");
    peers_[k] = comms[k]->impl_->slab.p;
    if (k != rank_) impl_->peer_engines[k] = pick_engines(impl_->own, impl_->own, k, epp_, engines_);
  }
  connected_ = true;
}

std::string SdmaComm::debug_state() const {
  std::string out = "epoch=" + std::to_string(epoch_) + " engines=";
  for (uint32_t e : sdma_engine_ids(engines_)) out += std::to_string(e) + ",";
  for (int k = 0; k < world_; ++k) {
    out += " peer" + std::to_string(k) + "_engines=";
    if (k < static_cast<int>(impl_->peer_engines.size()))
      for (auto e : impl_->peer_engines[k]) out += std::to_string(static_cast<uint32_t>(e)) + ",";
  }
  for (int i = 0; i < kSdmaSlots; ++i) {
    const Impl::Slot& sl = impl_->slots[i];
    if (!sl.used) continue;
    out += " | slot" + std::to_string(i) + " start=" + std::to_string(hsa_signal_load_relaxed(sl.start.s)) +
           " mid=";
    for (const Signal& x : sl.mid) out += std::to_string(hsa_signal_load_relaxed(x.s)) + ",";
    out += " scf=" + std::to_string(hsa_signal_load_relaxed(sl.scf.s)) +
           " gdf=" + std::to_string(hsa_signal_load_relaxed(sl.gdf.s));
  }
  std::vector<uint32_t> f(2 * kFrWord, 0);
  (void)hipMemcpy(f.data(), impl_->slab.p, f.size() * 4, hipMemcpyDeviceToHost);
  for (const char* what : {"FS", "FR"}) {
    out += std::string(" | ") + what + "[rank][piece]=";
    for (int k = 0; k < world_; ++k) {
      for (int q = 0; q < kSdmaMaxPieces; ++q)
        out += std::to_string(f[static_cast<size_t>(what[1] == 'S' ? sdma_fs_word(k, q) : sdma_fr_word(k, q))]) + ",";
      out += ";";
    }
  }
  return out;
}

uint32_t SdmaComm::error() const {
  uint32_t e = 0;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipMemcpy(&e, impl_->err.p, 4, hipMemcpyDeviceToHost), "hipMemcpy(err)");
  return e;
}

void SdmaComm::clear_error() {
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipMemset(impl_->err.p, 0, 4), "hipMemset(err)");
}

void SdmaComm::allreduce(const void* in, void* out, int64_t n, DType dt, hipStream_t stream, float scale) {
  allreduce_local({this}, {in}, {out}, n, dt, stream, scale);
}

// The ranks of one process on one stream: for each segment every rank's copies are queued
// first, then the stream releases every rank's phase 1, then ONE pipelined reduce launch for
// every local rank (blockIdx.y) and ONE pipelined gather launch. Each wait inside them only
// needs copies released before the launch, so one stream carries all local ranks.
void SdmaComm::allreduce_local(const std::vector<SdmaComm*>& comms, const std::vector<const void*>& ins,
                               const std::vector<void*>& outs, int64_t n, DType dt, hipStream_t stream, float scale) {
  if (comms.empty() || ins.size() != comms.size() || outs.size() != comms.size())
    throw std::invalid_argument("SdmaComm: one input and one output per local rank");
  SdmaComm& c0 = *comms[0];
  for (size_t y = 0; y < comms.size(); ++y) {
    const SdmaComm& c = *comms[y];
    if (!c.connected_) throw std::runtime_error("SdmaComm: connect() first");
    if (c.device_ != c0.device_ || c.world_ != c0.world_ || c.slot_bytes_ != c0.slot_bytes_ ||
        c.pieces_ != c0.pieces_ || c.grid_ != c0.grid_)
      throw std::invalid_argument("SdmaComm: local ranks must share device, world, slot size, pieces and grid");
    if ((reinterpret_cast<uintptr_t>(ins[y]) | reinterpret_cast<uintptr_t>(outs[y])) & 15)
      throw std::invalid_argument("SdmaComm: buffers must be 16-byte aligned");
  }
  if (n <= 0) return;
  hip_check(hipSetDevice(c0.device_), "hipSetDevice");
  const int64_t es = static_cast<int64_t>(dtype_size(dt));
  const int64_t seg = sdma_segment_elems(c0.world_, c0.slot_bytes_, es);
  const int W = c0.world_;
  std::vector<Plan> plans(comms.size());
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t len = std::min(seg, n - off);
    for (size_t y = 0; y < comms.size(); ++y)
      plans[y] = comms[y]->plan(static_cast<const char*>(ins[y]) + off * es, static_cast<char*>(outs[y]) + off * es,
                                len, es);
    hip_check(hipEventRecord(c0.impl_->sysrel.e, stream), "hipEventRecord(release to system)");
    for (size_t y = 0; y < comms.size(); ++y)
      launch_sdma_release(comms[y]->impl_->slots[plans[y].slot].start_p, stream);
    for (size_t y0 = 0; y0 < comms.size(); y0 += kSdmaMaxLocal) {
      const size_t ny = std::min<size_t>(kSdmaMaxLocal, comms.size() - y0);
      SdmaLaunch L{};
      L.n = len;
      L.block = plans[y0].seg.block;
      L.pe = plans[y0].seg.pe;
      L.K = plans[y0].seg.K;
      L.slot = c0.slot_bytes_;
      L.W = W;
      L.scale = scale;
      L.timeout = static_cast<uint64_t>(c0.timeout_s_ * 1e8);
      for (size_t i = 0; i < ny; ++i) {
        SdmaComm& c = *comms[y0 + i];
        const Plan& pl = plans[y0 + i];
        SdmaRankArgs& a = L.y[i];
        char* slab = c.impl_->slab.p;
        a.in = pl.in;
        a.out = pl.out;
        a.sd = slab + sdma_sd_off(W, c.slot_bytes_, pl.par, 0);
        a.rd = slab + sdma_rd_off(W, c.slot_bytes_, pl.par, 0);
        a.flags = reinterpret_cast<const uint32_t*>(slab);
        for (int k = 0; k < kSdmaMaxPieces; ++k) a.mid[k] = c.impl_->slots[pl.slot].mid_p[k];
        a.cnt = c.impl_->cnt.p;
        a.err = c.impl_->err.p;
        a.epoch = pl.epoch;
        a.r = c.rank_;
      }
      launch_sdma_reduce_gather(L, c0.grid_, static_cast<int>(ny), stream, dt);
    }
    hip_check(hipGetLastError(), "sdma kernels");
  }
}

// One segment in three steps: wait for the signal slot; the schedule (plan_sdma_copies); arm
// the signals to its counts and submit its copies in its order.
SdmaComm::Plan SdmaComm::plan(const char* in, char* out, int64_t n, int64_t es) {
  Impl& m = *impl_;
  Plan pl;
  pl.in = in;
  pl.out = out;
  const uint64_t e64 = ++epoch_;
  pl.epoch = static_cast<uint32_t>(e64);
  pl.par = static_cast<int>(e64 & 1u);
  pl.slot = static_cast<int>(e64 % kSdmaSlots);
  Impl::Slot& sl = m.slots[pl.slot];
  // the slot's previous call: every copy it submitted has completed (the host is at most
  // kSdmaSlots calls ahead of the engines; a peer that stopped turns into an error here)
  if (sl.used) {
    for (hsa_signal_t x : {sl.scf.s, sl.gdf.s}) {  // every part precedes a flag counted here
      if (hsa_signal_load_scacquire(x) == 0) continue;
      ++st_.host_waits;
      const uint64_t ns = static_cast<uint64_t>(timeout_s_ * 1e9);
      if (hsa_signal_wait_scacquire(x, HSA_SIGNAL_CONDITION_EQ, 0, ns, HSA_WAIT_STATE_BLOCKED) != 0)
        throw std::runtime_error("SdmaComm: copies of an earlier call did not complete (peer gone?)");
    }
  }
  sl.used = true;

  pl.seg = plan_sdma_segment(world_, n, es, slot_bytes_, pieces_);
  m.sched = plan_sdma_copies(pl.seg, world_, rank_, es, epp_, slot_bytes_, pl.par, std::move(m.sched));
  const SdmaSchedule& sc = m.sched;

  Impl::grow(sl.c1, sc.c1.size());
  Impl::grow(sl.c2, sc.c2.size());
  for (size_t i = 0; i < sc.c1.size(); ++i) hsa_signal_store_relaxed(sl.c1[i].s, sc.c1[i]);
  for (size_t k = 0; k < sc.c2.size(); ++k) hsa_signal_store_relaxed(sl.c2[k].s, sc.c2[k]);
  uint32_t* word = m.words.p + static_cast<int64_t>(pl.slot) * 16;
  *word = pl.epoch;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  hsa_signal_store_relaxed(sl.start.s, 1);
  for (int k = 0; k < kSdmaMaxPieces; ++k) hsa_signal_store_relaxed(sl.mid[k].s, 1);
  hsa_signal_store_relaxed(sl.scf.s, sc.scf);
  hsa_signal_store_relaxed(sl.gdf.s, sc.gdf);
  for (const SdmaCopy& c : sc.copies) {
    const bool flag = c.src == SdmaSrc::Epoch;
    const void* src = flag ? static_cast<const void*>(word) : (c.src == SdmaSrc::In ? in : out) + c.src_off;
    const hsa_signal_t dep = sl.of(c.dep);
    hsa_check(hsa_amd_memory_async_copy_on_engine(peers_[c.dst_rank] + c.dst_off, m.peer_agent[c.dst_rank], src,
                                                  flag ? m.cpu : m.own, static_cast<size_t>(c.bytes), 1, &dep,
                                                  sl.of(c.done), m.peer_engines[c.peer][c.engine], true),
              "hsa_amd_memory_async_copy_on_engine");
    ++st_.copies;
    st_.bytes += static_cast<uint64_t>(c.bytes);
  }
  ++st_.calls;
  return pl;
}

}  // namespace mxar
