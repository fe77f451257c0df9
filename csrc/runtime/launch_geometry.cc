#include "launch_geometry.h"

#include <algorithm>
#include <limits>
#include <stdexcept>
#include <string>

#include "../core/data_buffer.h"

namespace mxar {

static int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

int64_t flag_bytes(int world, int64_t slot_bytes, int threshold_rows, int64_t flag_gran) {
  const int rows = 1 + threshold_rows;
  if (flag_gran <= 0) flag_gran = min_chunk_bytes();
  const int64_t maxch = ceil_div(round_up(std::max<int64_t>(slot_bytes, 64 * 1024), 64 * 1024), flag_gran);
  // [F1: rows x P x maxch][F2: rows x P x maxch][FB: P][PROG: P][F2C: rows x P x maxch][FORCE: P]
  return (3 * rows * world * maxch + 3 * world) * 4;
}

SlabLayout slab_layout(int world, int64_t slot_bytes, int threshold_rows, int64_t min_flag_bytes, int64_t flag_gran,
                       int64_t ll_max) {
  SlabLayout L;
  const int rows = 1 + threshold_rows;
  if (flag_gran <= 0) flag_gran = min_chunk_bytes();
  L.slot_bytes = round_up(std::max<int64_t>(slot_bytes, 64 * 1024), 64 * 1024);
  L.maxch = ceil_div(L.slot_bytes, flag_gran);
  L.off_S = round_up(std::max(flag_bytes(world, slot_bytes, threshold_rows, flag_gran), min_flag_bytes), 64 * 1024);
  // Slots sit back to back (slot_stride = capacity). A pad that takes the P slots a reduce
  // reads off a power-of-two spacing showed no gain for the reduce kernel
  // (benchmarks/bench_reduce.py --pad-kib, profiles/reduce_kernel.md); its study knob was
  // removed in round 6.
  L.slot_stride = L.slot_bytes;
  L.off_R = L.off_S + rows * world * L.slot_stride;
  // low-latency one-shot slots: [2 parities][P sources] x ll_slot (two 8-B LL words per
  // 16-B store: ll_slot = 2 x payload)
  L.ll_max = round_up(ll_max, 16);
  L.ll_slot = round_up(std::max<int64_t>(2 * L.ll_max, 16), 64 * 1024);
  L.off_LL = L.off_R + rows * world * L.slot_stride;
  L.slab_bytes = L.off_LL + 2 * world * L.ll_slot;
  // Allocation size: on this ROCm stack hipIpcOpenMemHandle of an allocation whose size has
  // bit 31 set (2-4 GiB, 6-8 GiB, ...) never returns in the importing process, while the
  // sizes around it map and reduce correctly (measured with tools/ipc_size_probe.py, in git history: 1.97,
  // 4.05, 4.33 GiB fine; 2.03-3.9 GiB hang). Such slabs are padded up to the next multiple of
  // 4 GiB - at most 2 GiB of the 288 GB of HBM.
  L.alloc_bytes = ipc_safe_bytes(L.slab_bytes);
  return L;
}

int64_t ipc_safe_bytes(int64_t bytes) {
  if (bytes & (int64_t{1} << 31)) return round_up(bytes, int64_t{1} << 32);
  return bytes;
}

int launch_grid(const GridKnobs& k, int64_t bytes, bool oneshot, int64_t full_at) {
  // Workgroups for a two-shot / one-shot launch moving `bytes` of input (all ranks of the
  // launch). Every unit of work pays flag hand-offs and fenced stores without adding bytes
  // (PMC: 4x the workgroups at 8 x 1 MiB cost 8x the wait cycles, with no extra L2
  // write-back / invalidate operations), so below ~512 MiB per launch the full grid loses
  // to ~one workgroup per 64 KiB (8 / 4 / 2 logical ranks x 64 KiB - 256 MiB, same
  // box: two-shot 1 MiB x 8 ranks 36.6 -> 21.9 us, 16 MiB x 4 ranks 95.4 -> 67.8 us, 64 MiB x 2
  // ranks 132 -> 101 us, 256 MiB unchanged; profiles/round4/README.md section 9):
  //   two-shot: one workgroup per 64 KiB, 64..256, the full grid from `full_at` (512 MiB;
  //             the threshold kernel: 256 MiB - 4 x 64 MiB 288 us full vs 307 us sized);
  //   one-shot: every rank reads all P inputs, so one per 64 KiB of P x bytes, 64..full grid.
  // At the default grid only: an explicit grid is used as given.
  if (!k.size_grid || k.grid != k.default_grid) return k.grid;
  return size_grid_rule(bytes, k.grid, k.world, oneshot, full_at);
}

int shared_launch_cap(const GridKnobs& k, int ranks_here) {
  // Several logical ranks in one launch (one GPU): at most a quarter of the default grid - half
  // the CUs - per rank at the default grid. 2 ranks x 256 MiB bf16 two-shot 426-436 -> 389-395
  // us, threshold 432-440 -> 411-414; 4 x 128 MiB 128 per rank beats 64; 8 x 256 MiB equal
  // (profiles/round5/local_launch_grid.jsonl). One rank per GPU keeps launch_grid's rule.
  const int cap = shared_launch_rule(ranks_here, k.default_grid);
  if (cap <= 0 || !k.size_grid || k.grid != k.default_grid) return std::numeric_limits<int>::max();
  return cap;
}

int adamw_grid(const GridKnobs& k) {
  // the fused AdamW step (8 streams per element) runs best at 256 workgroups per device (134 M
  // params: 0.745 vs 0.762 ms at 512, same box, twice; profiles/round4/README.md section 5),
  // at the default grid
  return (k.size_grid && k.grid == k.default_grid) ? std::min(k.grid, 256) : k.grid;
}

int64_t block_elems(int world, int64_t n, int64_t es) { return round_up(ceil_div(n, world), 16 / es); }

// Workgroups per rank at most: all workgroups of the launch stay resident, so the device grid
// `gdev` is shared by the ranks of the launch.
static int per_rank(int gdev, int ranks_here) { return std::max(1, gdev / ranks_here); }

// flag_cols flag words per table row and block_bytes per slot must lie inside the slab
static void check_slab(const GridKnobs& k, int64_t flag_cols, int64_t block_bytes) {
  if (flag_cols > k.maxch || block_bytes > k.slot_bytes + 16)
    throw std::logic_error("XgmiComm: segment geometry exceeds slab");
}

LaunchGeometry plan_ll(const GridKnobs& k, int64_t n, int64_t es, int ranks_here) {
  LaunchGeometry g;
  const int gmax = per_rank(k.grid, ranks_here);
  const int64_t units = ceil_div(n * es, 8);
  g.block = g.chunk = g.subchunk = n;
  g.nch = 1;
  g.gx = static_cast<int>(std::min<int64_t>(gmax, std::max<int64_t>(1, ceil_div(units, kCommThreads))));
  return g;
}

LaunchGeometry plan_oneshot(const GridKnobs& k, int64_t n, int64_t es, int ranks_here) {
  LaunchGeometry g;
  const int64_t elems = 16 / es, min_chunk = min_chunk_bytes() / es;
  const int gmax = per_rank(launch_grid(k, n * es * ranks_here, true), ranks_here);
  g.block = n;
  g.chunk = std::max(min_chunk, round_up(ceil_div(n, gmax), elems));
  g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(n, g.chunk)));
  g.subchunk = g.chunk;
  g.gx = static_cast<int>(std::min<int64_t>(gmax, g.nch));
  check_slab(k, g.nch, g.block * es);
  return g;
}

LaunchGeometry plan_ring(const GridKnobs& k, int64_t n, int64_t es, int ranks_here, bool native) {
  // ring_depth chunks per workgroup, walked step-major (ring_kernel). Hop flags sit in the
  // row of the WRITER (the previous rank), one column block per hop: every flag word has a
  // single writer across all kernels, so epochs never go backwards (a ring's late forward
  // of launch e-1 landing on a word another rank's all-gather set to e lost that flag -
  // profiles/round3/README.md); (W - 1) * nch columns must fit the flag row.
  // Every hop of every workgroup pays a system-scope release and acquire, and those
  // serialise in the XCD's L2 when hundreds of workgroups fence at once: at 8 logical ranks
  // x 256 MiB the ring ran fastest with 256 workgroups in all (one per CU) and one chunk
  // per workgroup - more chunks per workgroup only multiply the fences (ring_grid sweep,
  // profiles/round4/README.md). MXAR_RING_GRID / MXAR_RING_DEPTH override.
  LaunchGeometry g;
  const int W = k.world;
  const int64_t elems = 16 / es, min_chunk = min_chunk_bytes() / es;
  const int gmax = per_rank(k.grid, ranks_here);
  const int depth = std::max(1, k.ring_depth);
  // and at the default grid, one workgroup per 32 KiB of the per-rank bytes, 64..ring_grid:
  // every hop of every workgroup is a dependent hand-off (8 / 2 logical ranks, ring_native
  // p50 at ring grid 64 / 128 / 256 / 512: 8 x 1 MiB 51 / 62 / 99 / 162 us, 8 x 4 MiB 108 / 96
  // / 136 / 250 us, 2 x 16 MiB 72 / 48 / 39 / 46 us; profiles/round4/ring_grid_mid.jsonl)
  int ring_dev = k.ring_grid;
  if (k.size_grid && k.grid == k.default_grid)
    ring_dev = static_cast<int>(std::min<int64_t>(k.ring_grid, std::max<int64_t>(64, n * es / (int64_t{32} << 10))));
  const int gring = std::max(1, std::min(gmax, ring_dev / ranks_here));
  g.block = round_up(ceil_div(n, W), elems);
  g.chunk = std::max(min_chunk, round_up(ceil_div(g.block, int64_t{gring} * depth), elems));
  g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(g.block, g.chunk)));
  const int64_t cols = std::max<int64_t>(1, k.maxch / std::max(1, W - 1));
  if (g.nch > cols) {
    g.chunk = round_up(ceil_div(g.block, cols), elems);
    g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(g.block, g.chunk)));
  }
  g.subchunk = g.chunk;
  g.gx = static_cast<int>(std::min<int64_t>(gring, g.nch));
  // the fp32 ring carries fp32 partials in its slots
  check_slab(k, static_cast<int64_t>(std::max(1, W - 1)) * g.nch, g.block * (native ? es : 4));
  return g;
}

LaunchGeometry plan_twoshot(const GridKnobs& k, int64_t n, int64_t es, int ranks_here, bool adamw) {
  // ~one scatter unit and one gather unit per workgroup: every unit pays one fence, so
  // units are as large as the parallelism allows. The reduce phase splits each chunk
  // W-1 ways to keep the same unit count.
  LaunchGeometry g;
  const int W = k.world;
  const int64_t elems = 16 / es, min_chunk = min_chunk_bytes() / es;
  // plain launches size the grid by their bytes (launch_grid)
  const int gdev = adamw ? adamw_grid(k) : launch_grid(k, n * es * ranks_here, false);
  const int gmax = std::min(per_rank(gdev, ranks_here), shared_launch_cap(k, ranks_here));
  g.block = round_up(ceil_div(n, W), elems);
  // Geometry by block size (same-box A/B over 2 / 4 / 8 logical ranks x 1-256 MiB,
  // profiles/round3/twoshot_geometry_ab.jsonl; MXAR_TWOSHOT_GEOM=coarse|fine|flat forces one):
  //   coarse (blocks < 2 MiB): ~one scatter unit per workgroup, each chunk reduced in up to
  //          P-1 pieces - fewest flag hand-offs, best while the round is latency bound;
  //   flat   (blocks >= 2 MiB): one chunk per workgroup (one reduce unit each, no split),
  //          the scatter in groups of `sgroup` chunks per destination (one copy and one
  //          release per group, a flag per chunk) - small chunks start the reduces early,
  //          grouped copies keep the scatter at copy speed: -22 % at 8 x 64 MiB, -7 % at
  //          8 x 256 MiB vs the best of the others, equal at 2 ranks;
  //   fine   (the round-2 choice for blocks >= 32 MiB): one chunk per workgroup for each of
  //          the P-1 destinations, reduced in 2 pieces - no longer the default.
  // an explicit units-per-workgroup (MXAR_TWOSHOT_UNITS, tune()'s "~1" labels) selects the
  // coarse / fine family it parameterises
  const int geom = k.geom >= 0 ? k.geom : k.units_per_wg > 0 ? 0 : (g.block * es >= k.flat_min ? 2 : 0);
  if (geom == 2 && W > 1) {
    g.chunk = std::max(min_chunk, round_up(ceil_div(g.block, gmax), elems));
    g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(g.block, g.chunk)));
    g.sub = 1;
    g.subchunk = g.chunk;
    g.gx = static_cast<int>(std::min<int64_t>(gmax, std::max<int64_t>(1, static_cast<int64_t>(W - 1) * g.nch)));
    const int per = std::max(1, g.gx / (W - 1));  // scatter groups per destination block
    g.sgroup = static_cast<int>(std::min<int64_t>(64, std::max<int64_t>(1, ceil_div(g.nch, per))));
  } else {
    const bool fine = geom == 1;
    const int upw = k.units_per_wg > 0 ? k.units_per_wg : fine ? std::max(1, W - 1) : 1;
    const int sub_max = k.sub_max > 0 ? k.sub_max : fine ? 2 : 64;
    const int64_t target = W > 1 ? std::max<int64_t>(1, int64_t{gmax} * upw / (W - 1)) : int64_t{gmax} * upw;
    g.chunk = std::max(min_chunk, round_up(ceil_div(g.block, target), elems));
    g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(g.block, g.chunk)));
    const int64_t sub = std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(W - 1), g.chunk / min_chunk, 64,
                                                                k.maxch / g.nch, int64_t{sub_max}}));
    g.subchunk = round_up(ceil_div(g.chunk, sub), elems);
    g.sub = static_cast<int>(ceil_div(g.chunk, g.subchunk));
    const int64_t units = std::max<int64_t>((W - 1) * static_cast<int64_t>(g.nch), static_cast<int64_t>(g.nch) * g.sub);
    g.gx = static_cast<int>(std::min<int64_t>(gmax, std::max<int64_t>(1, units)));
  }
  check_slab(k, static_cast<int64_t>(g.nch) * g.sub, g.block * es);
  return g;
}

LaunchGeometry plan_allreduce(Algo kind, const GridKnobs& k, int64_t n, int64_t es, int ranks_here, bool adamw) {
  switch (kind) {
    case Algo::LL: return plan_ll(k, n, es, ranks_here);
    case Algo::OneShot: return plan_oneshot(k, n, es, ranks_here);
    case Algo::Ring: return plan_ring(k, n, es, ranks_here, false);
    case Algo::RingNative: return plan_ring(k, n, es, ranks_here, true);
    default: return plan_twoshot(k, n, es, ranks_here, adamw);
  }
}

LaunchGeometry plan_coll(Coll op, const GridKnobs& k, int64_t n, int64_t es, int ranks_here) {
  LaunchGeometry g;
  const int W = k.world;
  const int64_t elems = 16 / es, min_chunk = min_chunk_bytes() / es;
  // launch-size grid as for the two-shot (launch_grid), over P x block bytes per rank: a
  // block goes to every peer (all-gather) or P blocks come in (all-to-all, reduce-scatter).
  // 8 / 2 logical ranks x 128 KiB - 8 MiB blocks, grid 64 - 512 (coll_grid_sweep.jsonl):
  // 8 x 512 KiB all-gather 58.4 -> 50.1 us, all-to-all 50.7 -> 41.2, reduce-scatter 44.9 ->
  // 35.4; the full grid pays off from 512 MiB (all-gather, all-to-all) / not yet at 512 MiB
  // for the reduce-scatter (8 x 8 MiB: 331 us full vs 284 us at 256).
  int gcap = per_rank(k.grid, ranks_here);
  if (k.size_grid && k.grid == k.default_grid) {
    const int64_t bytes = static_cast<int64_t>(ranks_here) * W * n * es;
    const int64_t full_at = op == Coll::ReduceScatter ? (int64_t{1} << 30) : (int64_t{512} << 20);
    if (bytes < full_at) gcap = std::max(1, size_grid_rule(bytes, k.grid, W, false, full_at) / ranks_here);
  }
  const int64_t target = std::max<int64_t>(1, gcap / (W - 1));
  g.chunk = std::max(min_chunk, round_up(ceil_div(n, target), elems));
  g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(n, g.chunk)));
  g.subchunk = g.chunk;
  g.sub = 1;
  if (op == Coll::ReduceScatter) {  // reduce units = push units: split every chunk W-1 ways
    const int64_t sub = std::max<int64_t>(1, std::min<int64_t>(W - 1, g.chunk / min_chunk));
    g.subchunk = round_up(ceil_div(g.chunk, sub), elems);
    g.sub = static_cast<int>(ceil_div(g.chunk, g.subchunk));
  }
  if (g.nch > k.maxch) throw std::logic_error("XgmiComm: collective geometry exceeds the flag table");
  g.gx = static_cast<int>(std::min<int64_t>(gcap, std::max<int64_t>(1, (W - 1) * int64_t{g.nch})));
  return g;
}

LaunchGeometry plan_rooted(Rooted kind, const GridKnobs& k, int64_t n, int64_t es, int ranks_here) {
  LaunchGeometry g;
  const int W = k.world;
  const int Wm1 = std::max(1, W - 1);
  const bool reduce = kind == Rooted::Reduce;
  const int64_t elems = 16 / es, min_chunk = min_chunk_bytes() / es;
  g.block = block_elems(W, n, es);
  // the launch-size grid of plan_coll over the P blocks of every rank in the launch, within the
  // shared-launch limits of the two-shot: all workgroups of the launch stay resident
  int gdev = k.grid;
  if (k.size_grid && k.grid == k.default_grid) {
    const int64_t bytes = static_cast<int64_t>(ranks_here) * W * g.block * es;
    const int64_t full_at = reduce ? (int64_t{1} << 30) : (int64_t{512} << 20);
    gdev = size_grid_rule(bytes, k.grid, W, false, full_at);
  }
  const int gcap = std::min(per_rank(gdev, ranks_here), shared_launch_cap(k, ranks_here));
  // ~one push unit per workgroup: a chunk goes to (or comes from) each of the P-1 peers
  const int64_t target = std::max<int64_t>(1, gcap / Wm1);
  g.chunk = std::max(min_chunk, round_up(ceil_div(g.block, target), elems));
  g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(g.block, g.chunk)));
  g.subchunk = g.chunk;
  g.sub = 1;
  if (reduce && g.nch <= k.maxch) {  // reduce units = push units, one flag column per reduce unit
    const int64_t sub =
        std::max<int64_t>(1, std::min<int64_t>({int64_t{Wm1}, g.chunk / min_chunk, k.maxch / g.nch}));
    g.subchunk = round_up(ceil_div(g.chunk, sub), elems);
    g.sub = static_cast<int>(ceil_div(g.chunk, g.subchunk));
  }
  g.gx = static_cast<int>(std::min<int64_t>(
      gcap, std::max<int64_t>({1, int64_t{Wm1} * g.nch, static_cast<int64_t>(g.nch) * g.sub})));
  check_slab(k, static_cast<int64_t>(g.nch) * g.sub, g.block * es);
  return g;
}

int round_grid(const GridKnobs& k, int nch) {
  // one reduce unit per workgroup where possible, and the scatter / gather units (P - 1 per
  // chunk) spread over as many workgroups as there are, up to the grid: a round of few
  // chunks otherwise serialises its hand-offs in one workgroup
  const int64_t units = static_cast<int64_t>(std::max(k.world - 1, 1)) * std::max(nch, 1);
  return static_cast<int>(std::min<int64_t>(k.grid, std::max<int64_t>({1, nch, units})));
}

// The threshold kernel's own geometry (data-parallel rounds).
static void threshold_geometry(const GridKnobs& k, int64_t n, int64_t es, int ranks_here, LaunchGeometry& g) {
  const int64_t elems = 16 / es, min_chunk = min_chunk_bytes() / es;
  // launch-size grid as for the two-shot (launch_grid; at the default grid only). The full
  // grid from 256 MiB per launch for one rank per device (round 4: 4 x 64 MiB 288 us full vs
  // 307 us sized); several logical ranks in one launch take it from 512 MiB like the two-shot
  // since round 6 (one reduce chunk per workgroup, 2 x 8 reduce batches): 4 x 64 MiB 271 ->
  // 248 us, 4 x 256 MiB 1066 -> 1040 us sized (profiles/round6 section 11)
  const int64_t full_at = ranks_here > 1 ? int64_t{512} << 20 : int64_t{256} << 20;
  const int gmax =
      std::min(std::max(1, launch_grid(k, n * es * std::max(1, ranks_here), false, full_at) / std::max(1, ranks_here)),
               shared_launch_cap(k, ranks_here));
  g.block = round_up(ceil_div(n, k.world), elems);
  // one reduce unit (a chunk: one threshold decision) per workgroup; phase 1/3 get P-1 each,
  // spread over up to (P - 1) x nch workgroups when the chunks are few (small tensors)
  g.chunk = std::max(min_chunk, round_up(ceil_div(g.block, gmax), elems));
  g.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(g.block, g.chunk)));
  g.gx = static_cast<int>(
      std::min<int64_t>(gmax, std::max<int64_t>(1, static_cast<int64_t>(std::max(k.world - 1, 1)) * g.nch)));
}

ThresholdPlan plan_threshold(const GridKnobs& k, int64_t n, int64_t es, int ranks_here, float thr, float thc,
                             const RoundShape& spec) {
  ThresholdPlan p;
  const int W = k.world;
  p.sub = 0;
  if (spec.block > 0) {  // the protocol's geometry (reference block ranges, maxChunkSize)
    if (spec.chunk <= 0) throw std::invalid_argument("round: chunk must be > 0");
    p.block = spec.block;
    p.chunk = spec.chunk;
    p.nch = static_cast<int>(std::max<int64_t>(1, ceil_div(p.block, p.chunk)));
    if (ranks_here != 1) throw std::invalid_argument("round: one rank per launch");
    p.gx = round_grid(k, p.nch);
    // Fewer chunks than workgroups (big maxChunkSize): split each chunk into slices of at
    // least 64 KiB, one workgroup each, until the reduce phase covers the grid. A chunk stays
    // ONE threshold decision (xgmi_threshold.hip, split chunks).
    const int64_t min_slice = std::max<int64_t>(64, (int64_t{64} << 10) / es);
    if (spec.split && W <= 30 && p.nch < k.grid && p.chunk >= 2 * min_slice) {
      const int64_t S = std::min<int64_t>(ceil_div(k.grid, p.nch), p.chunk / min_slice);
      if (S > 1) {
        p.subchunk = round_up(ceil_div(p.chunk, S), 64);
        p.sub = static_cast<int>(ceil_div(p.chunk, p.subchunk));
        const int64_t units = static_cast<int64_t>(p.nch) * p.sub;
        p.gx = static_cast<int>(
            std::min<int64_t>(k.grid, std::max<int64_t>(units, ceil_div(static_cast<int64_t>(W - 1) * units, 1024))));
        p.split = true;
      }
    }
  } else {
    threshold_geometry(k, n, es, ranks_here, p);
  }
  if (p.block * es > k.slot_bytes || p.nch > k.maxch)
    throw std::invalid_argument("allreduce_threshold: tensor exceeds one launch (n * dtype <= world * slot_bytes)");
  if (p.sub < 1) {  // unsplit: one workgroup per chunk
    p.sub = 1;
    p.subchunk = p.chunk;
  }
  // The reference's arrival order needs every reduce chunk of a workgroup in its launch
  // snapshot (xgmi_threshold.hip, S0); at thresholds 1 the order cannot change the result.
  if (spec.order_ref && !(thr >= 1.f && thc >= 1.f) &&
      ceil_div(static_cast<int64_t>(p.nch) * p.sub, p.gx) > kThresholdSnapChunks)
    throw std::invalid_argument("round: more than " + std::to_string(kThresholdSnapChunks) +
                                " chunks per workgroup at thresholds < 1 (the arrival-order snapshot)");
  // unsplit: scatter `sgroup` consecutive chunks per unit so that the (P - 1) x groups units
  // fit the grid once (at most 64: one flag lane each)
  p.sgroup = 1;
  if (p.sub <= 1 && W > 1) {
    const int per = std::max(1, p.gx / (W - 1));  // groups per destination block
    p.sgroup = static_cast<int>(std::min<int64_t>(64, std::max<int64_t>(1, ceil_div(p.nch, per))));
  }
  if (ceil_div(static_cast<int64_t>(W - 1) * p.nch * p.sub, p.gx) > kThresholdGatherUnits)
    throw std::invalid_argument("allreduce_threshold: more than " + std::to_string(kThresholdGatherUnits) +
                                " gather units per workgroup (too many chunks for the grid)");
  p.min_reduce = std::max(1, f32_threshold_count(thr, W));
  // thComplete: the reference's (th * P * nch) when every block has nch chunks; with a short
  // last block (uneven blocks) the chunks that exist, as the host WorkerCore
  // counts them (worker_core.cc) - the kernel never counts a chunk past a block's end
  int64_t total = 0;  // chunks that exist in the round
  {
    bool uniform = true;
    for (int j = 0; j < W; ++j) {
      const int64_t bl = std::max<int64_t>(0, std::min<int64_t>(p.block, n - static_cast<int64_t>(j) * p.block));
      const int64_t nc = ceil_div(bl, p.chunk);
      total += nc;
      uniform = uniform && nc == p.nch;
    }
    p.min_complete = uniform ? f32_threshold_chunks(thc, W, p.nch)
                             : std::max(1, f32_threshold_count(thc, static_cast<int>(total)));
  }
  p.full = (p.min_reduce >= W && thc >= 1.f) ? 1 : 0;
  // the lag-gate shortcut (xgmi_threshold.hip): rows for two rounds in flight, and a clean
  // round proves something about EVERY peer - each block holds a chunk, or nothing but a
  // complete round counts as clean (full thresholds)
  p.gate_shortcut =
      (k.rows - 1 >= 2 && (p.full || n > static_cast<int64_t>(W - 1) * p.block) && !k.no_gate_shortcut) ? 1 : 0;
  // the one-shot body (xgmi_threshold.hip): full thresholds, unsplit, a small round whose chunk
  // boundaries fall on 4-B words (a low-latency word is 4 payload bytes) and whose
  // LL-encoded input (two bytes of slot per byte) fits one S slot
  const int64_t nbytes = n * es;
  p.oneshot = (p.full && p.sub <= 1 && W <= kOneshotRanks && nbytes <= k.th_oneshot_max && nbytes % 4 == 0 &&
               (p.block * es) % 4 == 0 && (p.chunk * es) % 4 == 0 && 2 * round_up(nbytes, 8) <= k.slot_bytes)
                  ? 1
                  : 0;
  // the body reduces every chunk of the round (P x nch): as many chunks per workgroup as fit
  // its fast pass (one 8-B unit per thread, xgmi_threshold.hip), so the fewest workgroups
  // start (their start skew is on the round's critical path) and none walks chunks serially
  if (p.oneshot) {
    // each process decides from its local grid and cap (the open ADVICE item: make `cap` an
    // argument the membership agrees on)
    const int cap = ranks_here > 1 ? std::max(1, shared_launch_cap(k, ranks_here)) : k.grid;
    const int64_t upc = ceil_div(std::min(p.chunk, p.block) * es, 8) + 1;  // units of one chunk at most
    const int64_t cpw = std::max<int64_t>(1, kCommThreads / upc);
    const int64_t need = ceil_div(static_cast<int64_t>(W) * p.nch, cpw);
    // only where the grid holds a workgroup for each of those groups: a grid too small for
    // that (a small default grid, a shared launch's cap) left workgroups walking several
    // chunks chunk by chunk, which timed out (MXAR_GRID=64, 8 x 128 KiB; profiles/round6
    // section 12). One chunk of more than kCommThreads units per workgroup stays one-shot
    // (every workgroup walks its one chunk: the plane's coarsened forced rounds, T13).
    if (need > cap)
      p.oneshot = 0;
    else
      p.gx = static_cast<int>(need);
  }
  // lag skip: unsplit chunks (a split chunk's slices publish one flag between them, so they
  // would have to agree on the skip) and thresholds under which a round can complete
  // without one peer - its contribution (min_reduce < P) and its block's chunks
  // (min_complete within the other blocks' chunks)
  p.lag_skip =
      (spec.lag_skip && p.sub <= 1 && W >= 2 && p.min_reduce < W && p.min_complete <= total - p.nch) ? 1 : 0;
  return p;
}

}  // namespace mxar
