// Fused push-based allreduce over xGMI (gfx950). See xgmi_comm.h for the protocol map to
// the reference (AllreduceWorker.scala scatter/reduce/broadcast/complete).
//
// Slab layout (identical offsets on every rank, fine-grained device memory - the kind HSA
// makes coherent across agents during a kernel; MXAR_SLAB_MEM=uncached|coarse exist for
// study only: uncached slabs showed stale reads on MI355X, tests/test_comm_gpu.py stress):
//   [F1: P x maxch u32][F2: P x maxch u32][FB: P u32]  pad to 64 KiB
//   [S : P slots x slot_bytes]   S_k[s] = contribution of rank s to rank k's block
//   [R : P slots x slot_bytes]   R_k[j] = reduced block j, pushed by its owner j
// Flags hold the epoch of the launch that wrote them; epochs come from a device counter
// so launches replay correctly under hipGraph capture.
#include <hip/hip_runtime.h>

#include "xgmi_device.h"

namespace mxar {

// ---------------------------------------------------------------------------------
// Two-shot: direct reduce-scatter (push) + direct all-gather (push), one launch.
// ---------------------------------------------------------------------------------
template <class E, int PT>
__global__ __launch_bounds__(kCommThreads) void twoshot_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  const int P = PT > 0 ? PT : a.P;
  const int y = blockIdx.y;
  const int r = a.rank0 + y;
  const char* const in = a.in[y];
  char* const out = a.out[y];
  uint32_t* const ctl = a.ctl[y];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  const int G = gridDim.x;
  const int64_t slot = a.slot_bytes;
  uint32_t* err = &ctl[2];
  const bool rel = a.fence & 1, acq = a.fence & 2;
  const int Pm1 = P > 1 ? P - 1 : 1;
  const int nu = (P - 1) * a.nch;
  __shared__ uint64_t ps_lds[kPhaseSlots];
  PhaseStamps ps(a, ps_lds);

  // Phase 1 - ScatterBlock: push chunk c of block j to its owner j (rotated dest order,
  // AllreduceWorker.scala:194-209), so concurrent workgroups load all links. `sgroup`
  // consecutive chunks of one destination travel as ONE unit (one contiguous copy, one
  // release), each chunk keeping its own flag: small chunks pipeline the reduce, grouped
  // copies keep the scatter at copy speed ("flat" geometry, plan_twoshot).
  const int gs = a.sgroup > 1 ? a.sgroup : 1;
  const int nsu = Pm1 * ((a.nch + gs - 1) / gs);
  if (static_cast<int>(blockIdx.x) < nsu) entry_guard(a, ctl, r, epoch, kHazS, -1, deadline, err);  // block-uniform
  for (int u = blockIdx.x; u < nsu; u += G) {
    const int c0 = (u / Pm1) * gs;
    const int ncg = a.nch - c0 < gs ? a.nch - c0 : gs;
    const int j = (r + 1 + u % Pm1) % P;
    const int64_t bstart = static_cast<int64_t>(j) * a.block;
    const int64_t cstart = static_cast<int64_t>(c0) * a.chunk;
    const int64_t len = clamp_len(clamp_len(a.n - bstart, a.block) - cstart, static_cast<int64_t>(ncg) * a.chunk);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c0 + ncg - 1, err))
      copy_to_slab<E>(a.base[j] + a.off_S + r * slot + cstart * es, in + (bstart + cstart) * es, len);
    publish_flags([&](int i) { return f1(a, j, r, c0 + i); }, ncg, epoch, rel);
  }

  ps.mark(1);
  // Phase 2 - reduce own block once all P contributions of a chunk have arrived
  // (thReduce = 1), then ReduceBlock-broadcast the sum into every rank's R slot. A chunk
  // is reduced in `sub` pieces by different workgroups so that phase 2 has as many
  // units as phases 1 and 3 (each piece pays one acquire and one release). Units go to
  // workgroups by a static blockIdx stride (a counter-driven walk measured +1 % at 8 logical
  // ranks and slower at 2 - profiles/round4 - and was removed in round 6).
  const int64_t bstart_own = static_cast<int64_t>(r) * a.block;
  const int64_t blen_own = clamp_len(a.n - bstart_own, a.block);
  const int nu2 = a.nch * a.sub;
  for (int u = blockIdx.x; u < nu2; u += G) {
    const int c = u / a.sub;
    const int q = u % a.sub;
    const int64_t cbeg = static_cast<int64_t>(c) * a.chunk;
    const int64_t qbeg = static_cast<int64_t>(q) * a.subchunk;
    const int64_t cstart = cbeg + qbeg;
    const int64_t len = clamp_len(clamp_len(blen_own - cbeg, a.chunk) - qbeg, a.subchunk);
    const uint64_t tw = ps.now();
    wait_flags([&](int s) -> const uint32_t* { return s == r ? nullptr : f1(a, r, s, c); }, P, epoch, deadline, err,
               ERR_TIMEOUT_SCATTER, acq);
    ps.add(2, tw);
    ps.count(6);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, u, err)) {
      const char* own_in = in + (bstart_own + cstart) * es;
      const char* S = a.base[r] + a.off_S + cstart * es;
      char* own_out = out + (bstart_own + cstart) * es;
      const int64_t roff = a.off_R + r * slot + cstart * es;
      const RedSrc src{own_in, S, slot, r};
      reduce_to<E, PT>(P, src, P, r, [&](int k) -> char* { return k == r ? own_out : a.base[k] + roff; }, len,
                       a.scale, a.fence & 1);
    }
    publish_flags([&](int k) -> uint32_t* { return k == r ? nullptr : f2(a, k, r, u); }, P, epoch, rel);
  }

  ps.mark(3);
  read_delay(a, r);
  // Phase 3 - complete: gather the other owners' reduced chunks into the output. The
  // workgroup's units are polled together (wave 0, one lane per unit, up to 64 at a time)
  // and copied in ARRIVAL order: owners finish their reduces at different times, and a
  // workgroup waiting on its units one by one idles behind the latest of them while others
  // are ready (the threshold kernel's gather, which does this, was 13 % faster at 8 x 64 MiB
  // - profiles/round3/README.md).
  auto gather_unit = [&](int u) {
    const int c = u / Pm1;
    const int j = (r + 1 + u % Pm1) % P;
    const int64_t bstart = static_cast<int64_t>(j) * a.block;
    const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
    const int64_t len = clamp_len(clamp_len(a.n - bstart, a.block) - cstart, a.chunk);
    ps.count(7);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err))
      copy_from_slab<E>(out + (bstart + cstart) * es, a.base[r] + a.off_R + j * slot + cstart * es, len);
  };
  {
    __shared__ uint64_t arrived;
    __shared__ int late_s;
    const int mine = blockIdx.x < static_cast<unsigned>(nu) ? (nu - 1 - static_cast<int>(blockIdx.x)) / G + 1 : 0;
    for (int w0 = 0; w0 < mine; w0 += 64) {
      const int wn = mine - w0 < 64 ? mine - w0 : 64;
      uint64_t pending = wn == 64 ? ~0ull : ((1ull << wn) - 1ull);  // uniform across the workgroup
      const uint64_t tw = ps.now();
      while (pending) {
        if (threadIdx.x < 64) {
          const int lane = static_cast<int>(threadIdx.x);
          bool arr = false;
          if ((pending >> lane) & 1ull) {
            const int u = static_cast<int>(blockIdx.x) + (w0 + lane) * G;
            const int c = u / Pm1;
            const int j = (r + 1 + u % Pm1) % P;
            arr = true;
            for (int q = 0; q < a.sub && arr; ++q) arr = reached(ld_flag(f2(a, r, j, c * a.sub + q)), epoch);
          }
          const uint64_t m = __ballot(arr);
          const bool late = m == 0 && wall_ticks() > deadline;
          if (late && lane == 0) __hip_atomic_fetch_or(err, ERR_TIMEOUT_REDUCE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          if (m && acq) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope, once per batch
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) {
            arrived = m;
            late_s = late ? 1 : 0;
          }
        }
        __syncthreads();
        uint64_t m = arrived & pending;
        const bool late = late_s != 0;
        __syncthreads();
        if (late) break;  // the rest is given up (error word set, no data moved)
        if (!m) {
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        pending &= ~m;
        while (m) {
          const int i = __ffsll(static_cast<long long>(m)) - 1;
          m &= m - 1;
          gather_unit(static_cast<int>(blockIdx.x) + (w0 + i) * G);
        }
      }
      ps.add(4, tw);
    }
  }
  ps.mark(5);
  ps.flush();
  finish_launch_done(a, ctl, epoch, r, kHazR);  // peers may still gather from R
}

// ---------------------------------------------------------------------------------
// One-shot (latency path): every rank pushes its whole input into every peer's S slot,
// then reduces all P contributions locally - one xGMI hop instead of two.
// A push unit reads input chunk c ONCE and writes it to all P-1 peers, then publishes
// F1_k[r][c] for every k INCLUDING itself: the own flag means "chunk c of my input has
// been read", which the reduce of chunk c waits for before it may overwrite the input
// (in-place). The reduce reads its own contribution straight from the input.
// ---------------------------------------------------------------------------------
template <class E>
__device__ __forceinline__ void push_to_peers(const CommArgs& a, int P, int r, int64_t slot_off, const char* src,
                                              int64_t len) {
  const int64_t npk = len / E::ELEMS;
  const __amdgpu_buffer_rsrc_t rs = slab_rsrc(src);
  int64_t i = threadIdx.x;
  constexpr int U = 2;
  for (; i + (U - 1) * kCommThreads < npk; i += U * kCommThreads) {
    Pack16 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld16_nt(rs, static_cast<uint32_t>((i + u * kCommThreads) * 16));
    for (int k = 0; k < P; ++k) {
      if (k == r) continue;
      const __amdgpu_buffer_rsrc_t rd = slab_rsrc(a.base[k] + slot_off);
#pragma unroll
      for (int u = 0; u < U; ++u) st16_wt(rd, static_cast<uint32_t>((i + u * kCommThreads) * 16), v[u]);
    }
  }
  for (; i < npk; i += kCommThreads) {
    const Pack16 v = ld16_nt(rs, static_cast<uint32_t>(i * 16));
    for (int k = 0; k < P; ++k)
      if (k != r) st16_wt(slab_rsrc(a.base[k] + slot_off), static_cast<uint32_t>(i * 16), v);
  }
  const int64_t t = npk * E::ELEMS + threadIdx.x;
  if (t < len)
    for (int k = 0; k < P; ++k)
      if (k != r) copy_scalar_wt<E>(slab_rsrc(a.base[k] + slot_off), src, t);
}

template <class E, int PT>
__global__ __launch_bounds__(kCommThreads) void oneshot_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  const int P = PT > 0 ? PT : a.P;
  const int y = blockIdx.y;
  const int r = a.rank0 + y;
  const char* const in = a.in[y];
  char* const out = a.out[y];
  uint32_t* const ctl = a.ctl[y];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  const int G = gridDim.x;
  const int64_t slot = a.slot_bytes;
  uint32_t* err = &ctl[2];
  const bool rel = a.fence & 1, acq = a.fence & 2;
  // slots alternate between the S and R regions by epoch parity: a fast rank's next one-shot
  // pushes into the region its peers are NOT reading (no guard poll between one-shots)
  const bool odd = epoch & 1u;
  const int64_t region_off = odd ? a.off_R : a.off_S;
  const uint32_t region = odd ? kHazR : kHazS;
  if (static_cast<int>(blockIdx.x) < a.nch) entry_guard(a, ctl, r, epoch, region, -1, deadline, err);
  for (int c = blockIdx.x; c < a.nch; c += G) {
    const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
    const int64_t len = clamp_len(a.n - cstart, a.chunk);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err))
      push_to_peers<E>(a, P, r, region_off + r * slot + cstart * es, in + cstart * es, len);
    publish_flags([&](int k) { return f1(a, k, r, c); }, P, epoch, rel);
  }
  read_delay(a, r);
  for (int c = blockIdx.x; c < a.nch; c += G) {
    const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
    const int64_t len = clamp_len(a.n - cstart, a.chunk);
    wait_flags([&](int s) -> const uint32_t* { return f1(a, r, s, c); }, P, epoch, deadline, err, ERR_TIMEOUT_SCATTER,
               acq);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err)) {
      const RedSrc src{in + cstart * es, a.base[r] + region_off + cstart * es, slot, r};
      char* o = out + cstart * es;
      reduce_to<E, PT>(P, src, 1, 0, [&](int) -> char* { return o; }, len, a.scale, a.fence & 1);
    }
  }
  finish_launch_done(a, ctl, epoch, r, region);  // peers may still reduce from this region
}

// ---------------------------------------------------------------------------------
// Ring (BASELINE config 3's algorithm, kept for comparison and for topologies where only
// neighbour links are fast): reduce-scatter in P-1 hops + all-gather in P-1 hops, every
// hop a push into the next rank's slab. Each workgroup owns chunk c of every block and
// carries it around the whole ring, so all chunks are pipelined around the ring at once.
//   RS step s (0..P-2): send partial of block (r-s) into next's S[s][c], flag F1_next[s][c]
//                       (step 0 sends the raw input; step s>0 first adds S_r[s-1][c]).
//   final RS          : block (r+1) = S_r[P-2][c] + in[(r+1)][c], scaled once, to out and
//                       into next's R[0][c], flag F2_next[0][c].
//   AG step t (0..P-2): R_r[t][c] = block (r-t): copy to out, forward into next's R[t+1].
// Partial sums travel in fp32 whatever the element type (S slots hold fp32; a bf16 input is
// widened on the first hop), so a bf16 ring is rounded ONCE, at the final RS hop - as the
// two-shot is. For 16-bit types that costs 2x bytes on the RS hops and halves
// the elements one launch carries (XgmiComm::run segments by slot_bytes / 4 per block).
// Slot reuse across launches is safe: rank r's predecessor can only start the next launch
// after it received every block of this one, which transitively follows every read r
// makes of its S/R slots. One xGMI link per direction per rank carries the traffic.
// ---------------------------------------------------------------------------------
template <class E>
__device__ __forceinline__ void copy_slab_fwd(char* out, char* next_slab, const char* slab_src, int64_t len) {
  const int64_t npk = len / E::ELEMS;
  const __amdgpu_buffer_rsrc_t rs = slab_rsrc(slab_src);
  const __amdgpu_buffer_rsrc_t ro = slab_rsrc(out);
  const bool fwd = next_slab != nullptr;
  const __amdgpu_buffer_rsrc_t rn = slab_rsrc(fwd ? next_slab : out);
  int64_t i = threadIdx.x;
  constexpr int U = 4;
  for (; i + (U - 1) * kCommThreads < npk; i += U * kCommThreads) {
    Pack16 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld16_nt(rs, static_cast<uint32_t>((i + u * kCommThreads) * 16));
#pragma unroll
    for (int u = 0; u < U; ++u) st16_wt(ro, static_cast<uint32_t>((i + u * kCommThreads) * 16), v[u]);
    if (fwd) {
#pragma unroll
      for (int u = 0; u < U; ++u) st16_wt(rn, static_cast<uint32_t>((i + u * kCommThreads) * 16), v[u]);
    }
  }
  for (; i < npk; i += kCommThreads) {
    const Pack16 v = ld16_nt(rs, static_cast<uint32_t>(i * 16));
    st16_wt(ro, static_cast<uint32_t>(i * 16), v);
    if (fwd) st16_wt(rn, static_cast<uint32_t>(i * 16), v);
  }
  const int64_t t = npk * E::ELEMS + threadIdx.x;
  if (t < len) {
    const float x = ld_scalar_nt<E>(rs, t);
    st_scalar_wt<E>(ro, t, x);
    if (fwd) st_scalar_wt<E>(rn, t, x);
  }
}

// One ring hop. `partial` (a WT-typed slab slot, null on the first hop) + `in` (element type
// E), summed in fp32 -> either the next partial (`fwd_p`, write-through into the next rank's S
// slot, rounded to WT) or, on the final hop, scale x sum rounded once to E into `out` and the
// next rank's R slot (`fwd_e`). WT = F32 for a 16-bit E is the exact wire (partials travel
// in fp32, E::ELEMS / 4 fp32 packs per E pack); WT = E is the element-type wire (half the RS
// bytes, one extra rounding per intermediate hop). Two steps in flight per lane.
template <class E, class WT, int U>
__device__ __forceinline__ void ring_hop(const char* partial, const char* in, char* fwd_p, char* out, char* fwd_e,
                                         int64_t len, float scale) {
  constexpr bool wide = WT::ELEMS != E::ELEMS;
  constexpr int NP = wide ? E::ELEMS / 4 : 1;  // partial packs per E pack
  const int64_t npk = len / E::ELEMS;
  const bool has_p = partial != nullptr;
  const __amdgpu_buffer_rsrc_t rp = slab_rsrc(has_p ? partial : in);
  const __amdgpu_buffer_rsrc_t ri = slab_rsrc(in);
  const __amdgpu_buffer_rsrc_t rf = slab_rsrc(fwd_p != nullptr ? fwd_p : in);
  const __amdgpu_buffer_rsrc_t ro = slab_rsrc(out != nullptr ? out : in);
  const __amdgpu_buffer_rsrc_t re = slab_rsrc(fwd_e != nullptr ? fwd_e : in);
  // fp32 partial packs (wide wire) are laid out in planes of kCommThreads packs: for each run
  // of 256 E packs, NP planes of 256 fp32 packs - so every load / store instruction of a wave
  // covers 1 KiB of consecutive bytes (pack h of lane l at plane h, slot l). The plain layout
  // (lane l's NP packs side by side) gave each instruction every other 16 B of 2 KiB: twice
  // the lines per instruction, each half written. The last, short run is packed the same way
  // with `rows` slots per plane, so a chunk's partial stays inside its len x 4 bytes. Writer
  // and reader of a hop run this same function over the same len: the layout is private to
  // the ring's S slots.
  auto poff = [&](int64_t i, int h) -> uint32_t {
    const int64_t run = i / kCommThreads;
    const int64_t lane = i - run * kCommThreads;
    const int64_t left = npk - run * kCommThreads;
    const int64_t rows = left < kCommThreads ? left : kCommThreads;
    return static_cast<uint32_t>((run * kCommThreads * NP + h * rows + lane) * 16);
  };
  auto step = [&](int64_t i0, int nu) {
    Pack16 xv[U], pv[U][NP];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u >= nu) break;
      const int64_t i = i0 + u * kCommThreads;
      xv[u] = ld16_nt(ri, static_cast<uint32_t>(i * 16));
      if (has_p) {
#pragma unroll
        for (int h = 0; h < NP; ++h) pv[u][h] = ld16_nt(rp, wide ? poff(i, h) : static_cast<uint32_t>(i * 16));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u >= nu) break;
      const int64_t i = i0 + u * kCommThreads;
      Acc<E> acc;
      acc.zero();
      if (has_p) {
        if constexpr (wide) {
#pragma unroll
          for (int h = 0; h < NP; ++h)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc.v[4 * h + q] = __uint_as_float(pv[u][h][q]);
        } else {
          acc.add(pv[u][0]);
        }
      }
      acc.add(xv[u]);
      if (fwd_p != nullptr) {
        if constexpr (wide) {
#pragma unroll
          for (int h = 0; h < NP; ++h) {
            Pack16 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = __float_as_uint(acc.v[4 * h + q]);
            st16_wt(rf, poff(i, h), o);
          }
        } else {
          st16_wt(rf, static_cast<uint32_t>(i * 16), acc.pack());
        }
      } else {
        if (scale != 1.f) acc.scale(scale);
        const Pack16 o = acc.pack();
        st16_wt(ro, static_cast<uint32_t>(i * 16), o);
        if (fwd_e != nullptr) st16_wt(re, static_cast<uint32_t>(i * 16), o);
      }
    }
  };
  int64_t i = threadIdx.x;
  for (; i + (U - 1) * kCommThreads < npk; i += U * kCommThreads) step(i, U);
  for (; i < npk; i += kCommThreads) step(i, 1);
  const int64_t t = npk * E::ELEMS + threadIdx.x;
  if (t < len) {  // ragged tail: one element per lane
    float acc = (has_p ? ld_scalar_nt<WT>(rp, t) : 0.f) + ld_scalar_nt<E>(ri, t);
    if (fwd_p != nullptr) {
      st_scalar_wt<WT>(rf, t, acc);
    } else {
      acc *= scale;
      st_scalar_wt<E>(ro, t, acc);
      if (fwd_e != nullptr) st_scalar_wt<E>(re, t, acc);
    }
  }
}

// The workgroup's chunks are walked STEP-MAJOR: hop s of every chunk the workgroup owns
// (c = blockIdx.x + k * G) before hop s + 1 of any. The wait for chunk c at hop s then finds
// the predecessor's hop s - 1 of c long done (it was issued K - 1 chunks earlier), so flag
// latency and the ranks' jitter hide behind data movement instead of adding up over the
// 2 (P - 1) dependent hops of a chunk-major walk (round 3: 0.56 of the copy roofline at
// 8 logical ranks x 256 MiB bf16). Chunks per workgroup: XgmiComm ring_depth_.
template <class E, class WT, int U>
__global__ __launch_bounds__(kCommThreads) void ring_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  constexpr int ws = 16 / WT::ELEMS;  // wire bytes per element of a reduce-scatter partial
  const int P = a.P;
  const int y = blockIdx.y;
  const int r = a.rank0 + y;
  const int nxt = (r + 1) % P;
  const char* const in = a.in[y];
  char* const out = a.out[y];
  uint32_t* const ctl = a.ctl[y];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  const int64_t slot = a.slot_bytes;
  const int G = gridDim.x;
  uint32_t* err = &ctl[2];
  const bool rel = a.fence & 1, acq = a.fence & 2;
  __shared__ uint64_t ps_lds[kPhaseSlots];
  PhaseStamps ps(a, ps_lds);  // ring: [1] = end of the reduce-scatter hops, [2]/[4] = waits in RS / AG
  if (static_cast<int>(blockIdx.x) < a.nch) entry_guard(a, ctl, r, epoch, kHazS | kHazR, nxt, deadline, err);
  auto cst = [&](int c) { return static_cast<int64_t>(c) * a.chunk; };
  auto blen = [&](int b, int c) {
    return clamp_len(clamp_len(a.n - static_cast<int64_t>(b) * a.block, a.block) - cst(c), a.chunk);
  };
  auto at = [&](int b, int c) { return (static_cast<int64_t>(b) * a.block + cst(c)) * es; };
  // hop flags: rank k's word for hop h of chunk c, in the row of its only writer (k's
  // predecessor), one column block per hop. ring_hop_rows = the two-writer layout of round 3
  // (row = hop), a negative control only.
  const bool hop_rows = a.ring_hop_rows != 0;
  auto rs_flag = [&](int k, int h, int c) {
    return hop_rows ? f1(a, k, h, c) : f1(a, k, (k + P - 1) % P, h * a.nch + c);
  };
  auto ag_flag = [&](int k, int h, int c) {
    return hop_rows ? f2(a, k, h, c) : f2(a, k, (k + P - 1) % P, h * a.nch + c);
  };
  // every S access of chunk c is WT-typed [cstart, cstart + chunk), every R access E-typed;
  // the highest flag column is (P - 2) * nch + c. The geometry is the same on every rank,
  // so a chunk out of bounds is skipped by all of them (no flag is owed).
  auto inb = [&](int c) {
    return unit_in_bounds(a, cst(c) * ws, clamp_len(a.block - cst(c), a.chunk) * ws, (P - 2) * a.nch + c, err);
  };
  // RS hop 0: the raw own block r
  for (int c = blockIdx.x; c < a.nch; c += G) {
    if (!inb(c)) continue;
    const int64_t len = blen(r, c);
    if (len > 0) ring_hop<E, WT, U>(nullptr, in + at(r, c), a.base[nxt] + a.off_S + cst(c) * ws, nullptr, nullptr, len, 1.f);
    publish_flags([&](int) { return rs_flag(nxt, 0, c); }, 1, epoch, rel);
  }
  read_delay(a, r);  // slow-reader test knob: hold this rank before its first slab read
  // RS hops 1..P-1 (the last one completes block r+1 and starts its all-gather)
  for (int s = 1; s < P; ++s) {
    const int b = (r - s + P) % P;
    for (int c = blockIdx.x; c < a.nch; c += G) {
      if (!inb(c)) continue;
      const int64_t len = blen(b, c);
      const uint64_t tw = ps.now();
      wait_flags([&](int) -> const uint32_t* { return rs_flag(r, s - 1, c); }, 1, epoch, deadline, err,
                 ERR_TIMEOUT_SCATTER, acq);
      ps.add(2, tw);
      ps.count(6);
      const char* part = a.base[r] + a.off_S + (s - 1) * slot + cst(c) * ws;
      if (s < P - 1) {
        if (len > 0)
          ring_hop<E, WT, U>(part, in + at(b, c), a.base[nxt] + a.off_S + s * slot + cst(c) * ws, nullptr, nullptr, len,
                          1.f);
        publish_flags([&](int) { return rs_flag(nxt, s, c); }, 1, epoch, rel);
      } else {
        if (len > 0)
          ring_hop<E, WT, U>(part, in + at(b, c), nullptr, out + at(b, c), a.base[nxt] + a.off_R + cst(c) * es, len,
                          a.scale);
        publish_flags([&](int) { return ag_flag(nxt, 0, c); }, 1, epoch, rel);
      }
    }
  }
  ps.mark(1);
  read_delay(a, r);  // and before its first all-gather read
  // AG hops: receive block (r - t), forward unless it is the last hop
  for (int t = 0; t < P - 1; ++t) {
    const int b = (r - t + P) % P;
    const bool fwd = t < P - 2;
    for (int c = blockIdx.x; c < a.nch; c += G) {
      if (!inb(c)) continue;
      const int64_t len = blen(b, c);
      const uint64_t tw = ps.now();
      wait_flags([&](int) -> const uint32_t* { return ag_flag(r, t, c); }, 1, epoch, deadline, err,
                 ERR_TIMEOUT_REDUCE, acq);
      ps.add(4, tw);
      ps.count(7);
      if (fwd && t == P - 3) forward_delay(a, r);  // test knob: the last forward comes late
      char* d = fwd ? a.base[nxt] + a.off_R + (t + 1) * slot + cst(c) * es : nullptr;
      if (len > 0) copy_slab_fwd<E>(out + at(b, c), d, a.base[r] + a.off_R + t * slot + cst(c) * es, len);
      if (fwd) publish_flags([&](int) { return ag_flag(nxt, t + 1, c); }, 1, epoch, rel);
    }
  }
  ps.mark(3);
  ps.mark(5);
  ps.flush();
  finish_launch_done(a, ctl, epoch, r, kHazS | kHazR);  // the next rank may still read both
}

__global__ __launch_bounds__(kCommThreads) void barrier_kernel(CommArgs a) {
  const int r = a.rank0 + blockIdx.y;
  uint32_t* const ctl = a.ctl[blockIdx.y];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  publish_flags([&](int k) -> uint32_t* { return fb(a, k, r); }, a.P, epoch);
  wait_flags([&](int s) -> const uint32_t* { return fb(a, r, s); }, a.P, epoch, deadline, &ctl[2],
             ERR_TIMEOUT_BARRIER);
  finish_launch(ctl, epoch);
}

// ---------------------------------------------------------------------------------
// Host entries (XgmiComm, xgmi_comm.cc, fills the arguments)
// ---------------------------------------------------------------------------------
template <class E>
static void launch_typed(const CommArgs& a, dim3 grid, hipStream_t s, Algo kind) {
  const dim3 b(kCommThreads);
  // two packs in flight per lane and hop: 4 and 8 measured no faster (profiles/round5/ring_packs_in_flight_ab.jsonl)
  if (kind == Algo::Ring) {  // exact wire: fp32 partials
    hipLaunchKernelGGL((ring_kernel<E, F32, 2>), grid, b, 0, s, a);
    return;
  }
  if (kind == Algo::RingNative) {  // element-type wire
    hipLaunchKernelGGL((ring_kernel<E, E, 2>), grid, b, 0, s, a);
    return;
  }
  const bool oneshot = kind == Algo::OneShot;
#define MXAR_LAUNCH(PT)                                                                         \
  do {                                                                                          \
    if (oneshot)                                                                                \
      hipLaunchKernelGGL((oneshot_kernel<E, PT>), grid, b, 0, s, a);                            \
    else                                                                                        \
      hipLaunchKernelGGL((twoshot_kernel<E, PT>), grid, b, 0, s, a);                            \
  } while (0)
  switch (a.P) {
    case 1: MXAR_LAUNCH(1); break;
    case 2: MXAR_LAUNCH(2); break;
    case 4: MXAR_LAUNCH(4); break;
    case 8: MXAR_LAUNCH(8); break;
    default: MXAR_LAUNCH(0); break;
  }
#undef MXAR_LAUNCH
}

void launch_allreduce(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, Algo kind) {
  dispatch_dtype(static_cast<int>(dt), [&](auto tag) { launch_typed<decltype(tag)>(a, grid, s, kind); });
}

void launch_barrier(const CommArgs& a, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL(barrier_kernel, grid, dim3(kCommThreads), 0, s, a);
}

}  // namespace mxar
