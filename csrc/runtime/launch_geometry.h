// The launch geometry of every data-plane kernel (block, chunk, reduce pieces, workgroups) as
// pure functions of the communicator's knobs and the call's shape: no HIP, no environment, no
// device. XgmiComm (csrc/hip/xgmi_comm.cc) reads the environment once, hands its knobs in as
// values and copies the result into the kernel arguments; tests/test_launch_geometry.py pins
// every rule on the CPU against a table recorded from the code before the split, and
// csrc/tests/runtime_stress.cc checks the invariants the kernels rely on under sanitizers.
// Like plane_geometry: every shape bug the data plane has recorded was a host-side geometry
// decision, so the decisions live where they can run without a GPU.
#pragma once

#include <cstdint>

namespace mxar {

constexpr int kMaxRanks = 16;
// threshold kernel one-shot body: ranks at most (its per-source registers; larger memberships
// take the two-shot body)
constexpr int kOneshotRanks = 8;
// Threshold kernel: gather units (chunk x peer) one workgroup may own (its pending bitmap in
// LDS), and reduce chunks per workgroup with a launch snapshot (reference arrival order).
constexpr int kThresholdGatherUnits = 4096;
constexpr int kThresholdSnapChunks = 2048;
constexpr int kCommThreads = 256;
// Slot bytes per flag word at least, and the smallest chunk of every geometry.
constexpr int64_t min_chunk_bytes() { return 1024; }

// Ring: fp32 partials on the reduce-scatter hops (rounded once); RingNative: partials in the
// element type (half the RS wire bytes for 16-bit types, one rounding per hop).
enum class Algo : int { Auto = 0, TwoShot = 1, OneShot = 2, Ring = 3, LL = 4, RingNative = 5 };

// The reference's two allreduce phases as collectives of their own (xgmi_coll.hip).
enum class Coll : int { AllToAll = 0, AllGather = 1, ReduceScatter = 2 };

// The launch-size grid rule (launch_grid; profiles/round4/README.md section 9):
// workgroups for a launch moving `bytes` of input over all its ranks at device grid `grid`.
// Two-shot style: one per 64 KiB, 64..`cap`, the full grid from `full_at`; one-shot: every
// rank reads all `world` inputs, so one per 64 KiB of world x bytes, 64..the full grid.
inline int size_grid_rule(int64_t bytes, int grid, int world, bool oneshot, int64_t full_at = int64_t{512} << 20,
                          int64_t cap = 256) {
  if (oneshot) bytes *= (world > 1 ? world : 1);
  else if (bytes >= full_at) return grid;
  int64_t g = bytes / (int64_t{64} << 10);
  const int64_t hi = oneshot ? grid : cap;
  g = g < 64 ? 64 : (g > hi ? hi : g);
  return static_cast<int>(g < grid ? g : grid);
}

// Workgroups per rank at most when `ranks_here` logical ranks share one launch at the default
// grid (shared_launch_cap): a quarter of that grid, half the CUs. 0 = no cap.
inline int shared_launch_rule(int ranks_here, int default_grid) {
  return ranks_here <= 1 ? 0 : (default_grid / 4 > 1 ? default_grid / 4 : 1);
}

// Slab geometry for (world, slot_bytes, threshold_rows), without allocating.
struct SlabLayout {
  int64_t slot_bytes = 0, slot_stride = 0, maxch = 0, off_S = 0, off_R = 0, off_LL = 0, ll_max = 0, ll_slot = 0;
  int64_t slab_bytes = 0, alloc_bytes = 0;
};
// ll_max: largest tensor (bytes) one low-latency launch carries (MXAR_LL_MAX, read by XgmiComm)
SlabLayout slab_layout(int world, int64_t slot_bytes, int threshold_rows, int64_t min_flag_bytes, int64_t flag_gran,
                       int64_t ll_max);
// Bytes of the flag table alone (the part of off_S before its 64 KiB rounding).
int64_t flag_bytes(int world, int64_t slot_bytes, int threshold_rows, int64_t flag_gran);
// An allocation size hipIpcOpenMemHandle can map on this ROCm stack (see slab_layout).
int64_t ipc_safe_bytes(int64_t bytes);

// What the geometry rules read from a communicator (XgmiComm::knobs()).
struct GridKnobs {
  int world = 1;
  int rows = 1;  // S/R slot rows: 1 + threshold_rows
  // The device-default grid, and whether a launch at the default grid sizes it by its bytes
  // (launch_grid; MXAR_SIZE_GRID=0: always the full grid). An explicit grid (set_grid(g),
  // tune()'s "algo@g" labels) is always used as given.
  int grid = 512, default_grid = 512;
  bool size_grid = true;
  int64_t maxch = 0;       // flag words per table row (SlabLayout::maxch)
  int64_t slot_bytes = 0;  // capacity of one slot (SlabLayout::slot_bytes)
  int units_per_wg = 0;    // two-shot scatter units per workgroup; 0 = by block size (plan_twoshot)
  int sub_max = 0;         // two-shot: most reduce pieces per chunk; 0 = by block size
  int geom = -1;           // two-shot geometry: -1 by block size, 0 coarse, 1 fine, 2 flat (MXAR_TWOSHOT_GEOM)
  int64_t flat_min = int64_t{2} << 20;  // blocks of at least this many bytes use the flat geometry
  int ring_depth = 1;      // ring: chunks per workgroup, walked step-major (MXAR_RING_DEPTH)
  int ring_grid = 256;
  // full-threshold rounds of at most this many bytes per rank run the one-shot body
  // (xgmi_threshold.hip; MXAR_STUDY=1 MXAR_TH_ONESHOT_MAX=bytes, 0 = off): 1.1-1.8x faster
  // than the two-shot body at 64-256 KiB (profiles/round6 section 12). The multi-process
  // failures of a first 256 KiB default came from workgroups past the fast pass; the planner
  // sizes the grid for it or takes the two-shot body (plan_threshold)
  int64_t th_oneshot_max = 256 << 10;
  bool no_gate_shortcut = false;  // MXAR_STUDY=1 MXAR_GATE_SHORTCUT=0: threshold lag gate always polled (A/B)
};

// Workgroups of the device for a two-shot / one-shot launch moving `bytes` of input (all ranks
// of the launch).
int launch_grid(const GridKnobs& k, int64_t bytes, bool oneshot, int64_t full_at = int64_t{512} << 20);
// Workgroups per rank at most when several ranks share one launch (default grid only).
int shared_launch_cap(const GridKnobs& k, int ranks_here);
// Workgroups of the device for the fused AdamW step.
int adamw_grid(const GridKnobs& k);

// elements: block per rank, chunk (scatter / gather unit), subchunk (reduce unit); chunks per
// block, reduce units per chunk, chunks per scatter unit, workgroups per rank (gridDim.x)
struct LaunchGeometry {
  int64_t block = 0, chunk = 0, subchunk = 0;
  int nch = 0, sub = 1, sgroup = 0, gx = 1;
};

// One segment of n elements of `es` bytes, `ranks_here` logical ranks in the launch. Each
// throws std::logic_error where the geometry would not fit the slab.
LaunchGeometry plan_ll(const GridKnobs& k, int64_t n, int64_t es, int ranks_here);
LaunchGeometry plan_oneshot(const GridKnobs& k, int64_t n, int64_t es, int ranks_here);
LaunchGeometry plan_ring(const GridKnobs& k, int64_t n, int64_t es, int ranks_here, bool native);
// adamw: the fused reduce-scatter + AdamW + all-gather step (xgmi_adam.hip) on the same geometry
LaunchGeometry plan_twoshot(const GridKnobs& k, int64_t n, int64_t es, int ranks_here, bool adamw = false);
// kind: a resolved algorithm (not Auto)
LaunchGeometry plan_allreduce(Algo kind, const GridKnobs& k, int64_t n, int64_t es, int ranks_here,
                              bool adamw = false);
// One segment of n elements per block of a collective; `block` is the caller's (its m).
LaunchGeometry plan_coll(Coll op, const GridKnobs& k, int64_t n, int64_t es, int ranks_here);

// Rooted collectives (xgmi_rooted.hip): a broadcast is a scatter of the root's blocks plus an
// all-gather, a reduce a reduce-scatter plus a gather to the root.
enum class Rooted : int { Broadcast = 0, Reduce = 1 };
// One segment of n elements in all (block = block_elems(world, n, es) per rank). Broadcast
// chunks a block by plan_coll's all-gather rule, reduce by its reduce-scatter rule (each chunk
// reduced in `sub` pieces, one flag column per piece).
LaunchGeometry plan_rooted(Rooted kind, const GridKnobs& k, int64_t n, int64_t es, int ranks_here);

// Elements per block of a two-shot style launch: ceil(n / world) rounded to 16 B.
int64_t block_elems(int world, int64_t n, int64_t es);

// What plan_threshold reads of a protocol round (XgmiComm::RoundSpec); the default is a
// data-parallel round on the kernel's own geometry.
struct RoundShape {
  int64_t block = 0, chunk = 0;  // elements; 0: the kernel's own geometry
  bool order_ref = false;        // the reference's arrival-order accounting
  bool split = false;            // the round carries scratch to split its chunks over workgroups
  bool lag_skip = false;         // the round asks to skip a peer that is late at the lag gate
};
struct ThresholdPlan : LaunchGeometry {
  int min_reduce = 0;        // contributions per chunk that complete a reduce (thReduce)
  int64_t min_complete = 0;  // reduced chunks that complete the round (thComplete)
  int full = 0, gate_shortcut = 0, oneshot = 0, lag_skip = 0;
  bool split = false;        // chunks are split into `sub` slices (the scratch is used)
};
// Workgroups a protocol round of `nch` chunks per block uses.
int round_grid(const GridKnobs& k, int nch);
// Throws std::invalid_argument where the round does not fit one launch.
ThresholdPlan plan_threshold(const GridKnobs& k, int64_t n, int64_t es, int ranks_here, float th_reduce,
                             float th_complete, const RoundShape& spec = RoundShape());

}  // namespace mxar
