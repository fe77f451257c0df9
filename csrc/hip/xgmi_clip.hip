// The clipped sharded-data-parallel step over xGMI (gfx950): the fused step of xgmi_adam.hip
// split where a global gradient norm has to be known - after the reduce, before any parameter
// moves - into two launches on the same `adamw` geometry (plan_allreduce("adamw", ...)).
//
//   rs_sq_kernel       phases 1 and 2 of the fused step without the optimizer: scatter the
//                      gradient chunks to their owners; the owner sums the P contributions in
//                      fp32 in rank order, times `scale`, stores the fp32 value into its shard
//                      buffer `gshard` (block_elems elements, block `rank`; nothing past the valid
//                      length is written) and accumulates its square. The gradients are read
//                      with nt loads and never written. In its accumulating mode (template
//                      parameter ACC, gradient accumulation over micro-batches) it adds into
//                      the shard instead: gshard[i] = fl32(gshard[i] + fl32(scale * S[i])), the
//                      old value read with plain 16-B loads, and squares the new values.
//   adamw_shard_kernel phases 2 and 3 of the fused step with gshard[i] * coef as the gradient:
//                      the same adamw_unit (xgmi_adam_device.h: adamw(), the master rounded once,
//                      the write-through pushes to every peer) and gather. `coef` is one fp32 the
//                      host side computed on the device from every rank's sum of squares.
//
//                      In its record mode (template parameter REC, the loss-scaled step) coef,
//                      AdamW's bias corrections and a skip word come from the StepRecord the
//                      step-control kernel (xgmi_scale.hip) wrote between the halves.
//
// Between the two, 8 B per owned parameter go through HBM that the fused step keeps in
// registers (4 written, 4 read), and one 16-byte all-gather carries the ranks' sums.
//
// The sum of squares does not depend on the order workgroups arrive in; no floating-point
// atomics. Reduce unit u (chunk c, sub-unit q: L <= subchunk elements, one workgroup) sums
// through a fixed tree, with EL = elements per 16-B pack (4 fp32, 8 bf16 / fp16) and U = 2
// packs per lane per iteration:
//
//   lane       U * EL independent accumulators; accumulator (w, e) adds the squares of element
//              e of the packs tid + (2 k + w) * 256, k = 0, 1, ...: a chain of
//              iters(L) = ceil(floor(L / EL) / 512) additions
//   lane       the U * EL accumulators pairwise: log2(U * EL) levels (3 or 4); then the square
//              of the lane's element of the ragged tail (L mod EL elements): 1
//   wave       xor butterfly over the 64 lanes: 6 levels
//   workgroup  the 4 wave sums through LDS, (w0 + w1) + (w2 + w3): 2 levels
//
// and writes ONE partial to part[u]. The rank's last workgroup to finish (the ticket of
// finish_launch_done) adds part[0], part[1], ... in index order in double and rounds the sum
// once to fp32. Every term is non-negative, so the relative error of the result is at most
//
//   depth(L) * 2^-24,  depth(L) = iters(L) + log2(U * EL) + 12
//
// over the largest unit length L of the launch: 12 = 1 (the square) + 1 (tail) + 6 (wave) +
// 2 (workgroup) + 1 (the double sum over at most maxch units: < 2^-37 relative) + 1 (the
// rounding to fp32). At 2^28 elements per rank and the default grid (256 workgroups for one
// rank per device, so L = 2^20): fp32 527 * 2^-24 = 3.1e-5, 16-bit 272 * 2^-24 = 1.6e-5. An
// explicit grid of 8 workgroups (L = 2^25) gives 16399 * 2^-24 = 9.8e-4 for fp32; below 8
// workgroups per rank the bound passes 1e-3 for such a block. The accumulating mode feeds the
// NEW shard values through the same tree, unchanged: the bound counts the roundings of the tree
// from the stored fp32 values on, whatever produced them, so it holds there as it stands.
//
// Slot reuse: the reduce-scatter half follows the reduce-scatter of xgmi_coll.hip (entry guard
// on kHazS, the last workgroup tells the peers when this launch's S reads are done). The
// update half pushes into the peers' R slots without having heard from them in this launch,
// so - unlike the fused step, whose scatter phase proves every peer has entered the launch - it
// takes the entry guard on kHazR, and finishes like the fused step (peers may still gather).
#include <hip/hip_runtime.h>

#include "xgmi_adam_device.h"

namespace mxar {

namespace {

constexpr int kSqU = 2;  // packs per lane per iteration (the tree above)

// One reduce unit of the reduce-scatter half: gs[0, len) = scale * sum over ranks (fp32, rank
// order) and, for every thread, the unit's sum of squares through the tree above. All threads
// call; lds: 4 floats.
//
// ACC (gradient accumulation): gs[i] = fl32(gs[i] + fl32(scale * S[i])) and the squares are those
// of the new values. The product is rounded to fp32 BEFORE the add: left to itself the compiler
// contracts a * b + c into one fma, whose single rounding differs from the two roundings of
// plain fp32 ops wherever scale is no power of two (1/3, 1/5), and the accumulated shard would
// no longer be what `old + plain` gives in torch fp32 on any device. The empty asm pins the
// product as an fp32 register value (the idiom of adamw(), xgmi_adam_device.h); no instruction.
// The old values come in with plain 16-B loads (just written by the previous micro-batch, read
// again by the update half: not nt), issued with the gradient loads before the first use.
template <class E, int PT, bool ACC>
__device__ __forceinline__ float reduce_sq_unit(int P, const RedSrc& src, float* gs, int64_t len, float scale,
                                                float* lds) {
  constexpr int EL = E::ELEMS;
  constexpr int U = kSqU;
  const int64_t npk = len / EL;
  float sq[U * EL];
#pragma unroll
  for (int k = 0; k < U * EL; ++k) sq[k] = 0.f;
  for (int64_t i0 = threadIdx.x; i0 < npk; i0 += U * kCommThreads) {
    Acc<E> acc[U];
    float4 old[U][ACC ? EL / 4 : 1];
    bool live[U];
#pragma unroll
    for (int w = 0; w < U; ++w) {
      const int64_t i = i0 + w * kCommThreads;
      live[w] = i < npk;
      acc[w].zero();
      if (!live[w]) continue;
      if constexpr (ACC) {
#pragma unroll
        for (int e = 0; e < EL / 4; ++e) old[w][e] = *reinterpret_cast<const float4*>(gs + i * EL + 4 * e);
      }
      if constexpr (PT > 0) {
        Pack16 g[PT];
#pragma unroll
        for (int s = 0; s < PT; ++s) g[s] = ld16_nt(src.rsrc(s), static_cast<uint32_t>(i * 16));
#pragma unroll
        for (int s = 0; s < PT; ++s) acc[w].add(g[s]);
      } else {
        for (int s = 0; s < P; ++s) acc[w].add(ld16_nt(src.rsrc(s), static_cast<uint32_t>(i * 16)));
      }
    }
#pragma unroll
    for (int w = 0; w < U; ++w) {
      if (!live[w]) continue;
      const int64_t i = i0 + w * kCommThreads;
#pragma unroll
      for (int e = 0; e < EL; ++e) {
        float g = acc[w].v[e] * scale;
        if constexpr (ACC) {
          asm("" : "+v"(g));  // fl32(scale * S) first: no fma
          g += reinterpret_cast<const float*>(&old[w][e / 4])[e % 4];
        }
        acc[w].v[e] = g;
        sq[w * EL + e] += g * g;
      }
      // plain stores: the two 16-B halves of a 16-bit pack's 32 B merge in L2
#pragma unroll
      for (int e = 0; e < EL / 4; ++e)
        *reinterpret_cast<float4*>(gs + i * EL + 4 * e) =
            make_float4(acc[w].v[4 * e], acc[w].v[4 * e + 1], acc[w].v[4 * e + 2], acc[w].v[4 * e + 3]);
    }
  }
#pragma unroll
  for (int s = U * EL / 2; s >= 1; s /= 2)
#pragma unroll
    for (int k = 0; k < s; ++k) sq[k] += sq[k + s];
  float lane = sq[0];
  const int64_t t = npk * EL + threadIdx.x;
  float tail = 0.f;
  if (t < len) {
    float g = 0.f;
    float old_t = 0.f;
    if constexpr (ACC) old_t = gs[t];
    for (int s = 0; s < P; ++s) g += ld_scalar_nt<E>(src.rsrc(s), t);
    g *= scale;
    if constexpr (ACC) {
      asm("" : "+v"(g));
      g += old_t;
    }
    gs[t] = g;
    tail = g * g;
  }
  lane += tail;
#pragma unroll
  for (int m = 32; m >= 1; m /= 2) lane += __shfl_xor(lane, m, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = lane;
  __syncthreads();
  const float total = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();  // lds is written again by the workgroup's next unit
  return total;
}

// finish_launch_done (xgmi_device.h) with the rank's sum of squares formed by the last workgroup
// to finish: every workgroup's partials were stored with agent-scope atomics by its thread 0,
// which then releases (agent scope) before it takes the ticket; the last workgroup acquires
// after the ticket and adds the partials in index order, in double, rounded once to fp32.
__device__ __forceinline__ void finish_launch_sq(const CommArgs& a, uint32_t* ctl, uint32_t epoch, int r,
                                                 const float* part, int nparts, float* sq_out) {
  __shared__ int last;
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const uint32_t t = __hip_atomic_fetch_add(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = t == gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!last) return;
  const int k = static_cast<int>(threadIdx.x);
  if (k < a.P && k != r) st_flag(fb(a, k, r), epoch);
  if (threadIdx.x < 64) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double total = 0.0;
    for (int base = 0; base < nparts; base += 64) {
      const int idx = base + k;
      const float v = idx < nparts ? __hip_atomic_load(&part[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
#pragma unroll
      for (int l = 0; l < 64; ++l)  // index order; +0 past the end
        total += static_cast<double>(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)));
    }
    if (k == 0) *sq_out = static_cast<float>(total);
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&ctl[12], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // kHazS
    __hip_atomic_store(&ctl[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctl[0], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

template <class E, int PT, bool ACC>
__global__ __launch_bounds__(kCommThreads) void rs_sq_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  __shared__ float wave_sq[4];
  const StepCtx k(a, PT > 0 ? PT : a.P);
  const int y = blockIdx.y;
  const int r = k.r;
  const char* const grad = a.in[y];
  const int64_t slot = a.slot_bytes;  // read once, here: see twoshot_adamw_kernel (xgmi_adam.hip)
  float* const gshard = a.gshard[y];
  float* const part = a.sq_part[y];

  // Phase 1 - gradient ScatterBlock: chunk c of block j to its owner j
  if (static_cast<int>(blockIdx.x) < k.nu) entry_guard(a, k.ctl, r, k.epoch, kHazS, -1, k.deadline, k.err);
  scatter_grads<E>(a, k, grad);

  read_delay(a, r);
  // Phase 2 - reduce own chunk into the fp32 shard, one partial sum of squares per unit
  const int64_t bstart_own = static_cast<int64_t>(r) * a.block;
  const int nu2 = a.nch * a.sub;
  for (int u = blockIdx.x; u < nu2; u += k.G) {
    const OwnUnit o = own_unit(a, r, u);
    wait_flags([&](int s) -> const uint32_t* { return s == r ? nullptr : f1(a, r, s, o.c); }, k.P, k.epoch, k.deadline,
               k.err, ERR_TIMEOUT_SCATTER, k.acq);
    float usq = 0.f;  // an empty unit's partial
    if (o.len > 0 && unit_in_bounds(a, o.cstart * es, o.len * es, u, k.err)) {
      const RedSrc src{grad + (bstart_own + o.cstart) * es, a.base[r] + a.off_S + o.cstart * es, slot, r};
      usq = reduce_sq_unit<E, PT, ACC>(k.P, src, gshard + o.cstart, o.len, a.scale, wave_sq);
    }
    if (threadIdx.x == 0) __hip_atomic_store(&part[u], usq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  finish_launch_sq(a, k.ctl, k.epoch, r, part, nu2, a.sq_out[y]);  // peers may still reduce what was pushed into S
}

// The update half: phases 2 and 3 of the fused step through the same adamw_unit and
// gather_params (xgmi_adam_device.h), with the fp32 shard times the clip coefficient as the
// gradient. tests/test_clip_gpu.py holds the two gradient sources bit for bit against each other.
//
// REC (the loss-scaled step, xgmi_scale.hip): a.coef[y] points at the rank's StepRecord. The
// coefficient and AdamW's two bias corrections come from it instead of the launch arguments, and
// its skip word decides whether the launch updates anything. The record was written by the
// control kernel earlier on the same stream and is read with plain loads; it is uniform over the
// launch, and it has the same bits on every rank (the control kernels add the same records in the
// same order), so every rank takes the same branch.
//
// A skipped launch writes no master, moment or parameter, no R slot of a peer, and gathers
// nothing: the reduce units and the copy out of the R slots are left out. It still walks the whole
// flag protocol - the entry guard, the epoch-e flag of every reduce unit to every peer, the wait
// for every peer's flags, the last workgroup's "launch e done" - and that is on purpose. Every
// kernel of a communicator leans on one invariant (entry_guard, xgmi_device.h): a rank that has
// completed launch e has seen epoch-e flags from every peer, so every peer has entered e and
// finished every launch before it; "only the previous launch's reads can still be pending" is
// that sentence. A skipped launch that left through the finish path alone would complete
// without hearing from anyone: after rs_sq at e - 1 (kHazS = e - 1) and a skipped e, the next
// reduce-scatter half at e + 1 finds kHazS != e and pushes unguarded into S slots a slower peer
// is still reducing in e - 1; the low-latency kernel's parity slots of e and e + 2 would meet the
// same way. Carrying the hazard words forward could mend the first case and not the second. With
// the protocol walked, a skipped launch is to every other kernel an ordinary update half that
// happened to move no data: epoch, ticket, kHazR and the flag rows end exactly as after a clean
// one (kHazR is recorded although no R slot was read: a poll of one local word per peer at most).
// The flags of a skipped launch promise R data that was never pushed; only the same launch's
// gather could take them, and it reads no slot. Cost: the flag round trip, about the latency
// of an empty launch of this grid.
template <class E, int STREAM, int U, bool REC>
__global__ __launch_bounds__(kCommThreads) void adamw_shard_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  const StepCtx k(a, a.P);
  const int y = blockIdx.y;
  const int r = k.r;
  const float* const gshard = a.gshard[y];
  StepRecord rec{};
  if constexpr (REC)
    rec = *reinterpret_cast<const StepRecord*>(a.coef[y]);
  else
    rec.coef = *a.coef[y];
  const bool skip = REC && rec.skip != 0;  // uniform

  // AdamW on the owned shard, push the new parameters (phase 2 of the fused step). The pushes
  // go into R slots the peers may still be reading in the previous launch: entry guard.
  const int nu2 = a.nch * a.sub;
  if (k.P > 1 && static_cast<int>(blockIdx.x) < nu2) entry_guard(a, k.ctl, r, k.epoch, kHazR, -1, k.deadline, k.err);
  for (int u = blockIdx.x; u < nu2; u += k.G) {
    const OwnUnit o = own_unit(a, r, u);
    if (!skip && o.len > 0 && unit_in_bounds(a, o.cstart * es, o.len * es, u, k.err)) {
      if constexpr (REC)
        adamw_unit<E, STREAM, U>(a, k.P, r, o.cstart, o.len, RecordGrad<E>(slab_rsrc(gshard + o.cstart), rec));
      else
        adamw_unit<E, STREAM, U>(a, k.P, r, o.cstart, o.len, ShardGrad<E>{slab_rsrc(gshard + o.cstart), rec.coef});
    }
    publish_flags([&](int p) -> uint32_t* { return p == r ? nullptr : f2(a, p, r, u); }, k.P, k.epoch, k.rel);
  }

  // Gather the other owners' updated parameter chunks (phase 3 of the fused step); a skipped
  // launch only waits for their flags
  if (skip) {
    for (int u = blockIdx.x; u < k.nu; u += k.G) {
      const PeerUnit p = peer_unit(a, k, u);
      wait_flags([&](int q) -> const uint32_t* { return f2(a, k.r, p.j, p.c * a.sub + q); }, a.sub, k.epoch,
                 k.deadline, k.err, ERR_TIMEOUT_REDUCE, k.acq);
    }
  } else {
    gather_params<E>(a, k, a.out[y]);
  }
  finish_launch_done(a, k.ctl, k.epoch, r, kHazR);  // peers may still gather from R
}

namespace {

template <class E, bool ACC>
void launch_rs_sq_mode(const CommArgs& a, dim3 grid, hipStream_t s) {
  // static P as in launch_adamw: every source's load issues before the first add
  switch (a.P) {
    case 1: hipLaunchKernelGGL((rs_sq_kernel<E, 1, ACC>), grid, dim3(kCommThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL((rs_sq_kernel<E, 2, ACC>), grid, dim3(kCommThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL((rs_sq_kernel<E, 4, ACC>), grid, dim3(kCommThreads), 0, s, a); break;
    case 8: hipLaunchKernelGGL((rs_sq_kernel<E, 8, ACC>), grid, dim3(kCommThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((rs_sq_kernel<E, 0, ACC>), grid, dim3(kCommThreads), 0, s, a); break;
  }
}

}  // namespace

void launch_rs_sq(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, bool accumulate) {
  dispatch_dtype(static_cast<int>(dt), [&](auto tag) {
    using E = decltype(tag);
    if (accumulate)
      launch_rs_sq_mode<E, true>(a, grid, s);
    else
      launch_rs_sq_mode<E, false>(a, grid, s);
  });
}

namespace {

template <bool REC>
void launch_adamw_shard_mode(const CommArgs& a, dim3 grid, hipStream_t s, DType dt) {
  dispatch_dtype(static_cast<int>(dt), [&](auto tag) {
    using E = decltype(tag);
    // 16-bit parameters: run-contiguous halves; fp32: the generic body, plain state access
    if constexpr (E::ELEMS == 8)
      hipLaunchKernelGGL((adamw_shard_kernel<E, 3, 2, REC>), grid, dim3(kCommThreads), 0, s, a);
    else
      hipLaunchKernelGGL((adamw_shard_kernel<E, 0, 2, REC>), grid, dim3(kCommThreads), 0, s, a);
  });
}

}  // namespace

void launch_adamw_shard(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, bool record) {
  if (record)
    launch_adamw_shard_mode<true>(a, grid, s, dt);
  else
    launch_adamw_shard_mode<false>(a, grid, s, dt);
}

}  // namespace mxar
