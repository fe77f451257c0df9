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
//                      the same adamw() (xgmi_adam_device.h), the master rounded once, the
//                      write-through pushes to every peer, the gather. `coef` is one fp32 the
//                      host side computed on the device from every rank's sum of squares.
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
  const int P = PT > 0 ? PT : a.P;
  const int y = blockIdx.y;
  const int r = a.rank0 + y;
  const char* const grad = a.in[y];
  float* const gshard = a.gshard[y];
  float* const part = a.sq_part[y];
  uint32_t* const ctl = a.ctl[y];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  const int G = gridDim.x;
  const int64_t slot = a.slot_bytes;
  uint32_t* err = &ctl[2];
  const bool rel = a.fence & 1, acq = a.fence & 2;
  const int Pm1 = P > 1 ? P - 1 : 1;
  const int nu = (P - 1) * a.nch;

  // Phase 1 - gradient ScatterBlock: chunk c of block j to its owner j
  if (static_cast<int>(blockIdx.x) < nu) entry_guard(a, ctl, r, epoch, kHazS, -1, deadline, err);
  for (int u = blockIdx.x; u < nu; u += G) {
    const int c = u / Pm1;
    const int j = (r + 1 + u % Pm1) % P;
    const int64_t bstart = static_cast<int64_t>(j) * a.block;
    const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
    const int64_t len = clamp_len(clamp_len(a.n - bstart, a.block) - cstart, a.chunk);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err))
      copy_to_slab<E>(a.base[j] + a.off_S + r * slot + cstart * es, grad + (bstart + cstart) * es, len);
    publish_flags([&](int) { return f1(a, j, r, c); }, 1, epoch, rel);
  }

  read_delay(a, r);
  // Phase 2 - reduce own chunk into the fp32 shard, one partial sum of squares per unit
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
    wait_flags([&](int s) -> const uint32_t* { return s == r ? nullptr : f1(a, r, s, c); }, P, epoch, deadline, err,
               ERR_TIMEOUT_SCATTER, acq);
    float usq = 0.f;  // an empty unit's partial
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, u, err)) {
      const RedSrc src{grad + (bstart_own + cstart) * es, a.base[r] + a.off_S + cstart * es, slot, r};
      usq = reduce_sq_unit<E, PT, ACC>(P, src, gshard + cstart, len, a.scale, wave_sq);
    }
    if (threadIdx.x == 0) __hip_atomic_store(&part[u], usq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  finish_launch_sq(a, ctl, epoch, r, part, nu2, a.sq_out[y]);  // peers may still reduce what was pushed into S
}

// The update half. The body of a reduce unit is the text of twoshot_adamw_kernel's (xgmi_adam.hip)
// written in the kernel as it is there, with ONE gradient source - the fp32 shard, summed into the
// zeroed accumulator through the loops of the fused step's P-way sum - and the coefficient where
// the fused step has its scale: the compiler orders and contracts the products of adamw() by
// the code around them, and only the same text in the same place gave the fused step's bits
// (tests/test_clip_gpu.py holds the two kernels bit for bit against each other).
template <class E, int STREAM, int U>
__global__ __launch_bounds__(kCommThreads) void adamw_shard_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  constexpr int EL = E::ELEMS;
  constexpr int PT = 1;  // gradient sources
  const int P = a.P;
  const int y = blockIdx.y;
  const int r = a.rank0 + y;
  const float* const gshard = a.gshard[y];
  const float coef = *a.coef[y];
  char* const param = a.out[y];
  float* const mp = a.opt_p[y];
  float* const m1 = a.opt_m[y];
  float* const m2 = a.opt_v[y];
  uint32_t* const ctl = a.ctl[y];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  const int G = gridDim.x;
  const int64_t slot = a.slot_bytes;
  uint32_t* err = &ctl[2];
  const bool rel = a.fence & 1, acq = a.fence & 2;
  const int Pm1 = P > 1 ? P - 1 : 1;
  const int nu = (P - 1) * a.nch;

  // AdamW on the owned shard, push the new parameters (phase 2 of the fused step). The pushes
  // go into R slots the peers may still be reading in the previous launch: entry guard.
  const int64_t bstart_own = static_cast<int64_t>(r) * a.block;
  const int64_t blen_own = clamp_len(a.n - bstart_own, a.block);
  const int nu2 = a.nch * a.sub;
  if (P > 1 && static_cast<int>(blockIdx.x) < nu2) entry_guard(a, ctl, r, epoch, kHazR, -1, deadline, err);
  for (int u = blockIdx.x; u < nu2; u += G) {
    const int c = u / a.sub;
    const int q = u % a.sub;
    const int64_t cbeg = static_cast<int64_t>(c) * a.chunk;
    const int64_t qbeg = static_cast<int64_t>(q) * a.subchunk;
    const int64_t cstart = cbeg + qbeg;
    const int64_t len = clamp_len(clamp_len(blen_own - cbeg, a.chunk) - qbeg, a.subchunk);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, u, err)) {
      const __amdgpu_buffer_rsrc_t rg = slab_rsrc(gshard + cstart);  // read once: nt loads
      char* own_out = param + (bstart_own + cstart) * es;
      const int64_t roff = a.off_R + r * slot + cstart * es;
      float* const sp = mp + cstart;
      float* const sm = m1 + cstart;
      float* const sv = m2 + cstart;
      const __amdgpu_buffer_rsrc_t rp = slab_rsrc(sp), rm = slab_rsrc(sm), rv = slab_rsrc(sv);
      const int64_t npk = len / EL;
      if constexpr (STREAM == 3 && EL == 8) {
        // Run-contiguous halves (16-bit parameters, the default): lane l of a run of 256 packs
        // takes elements [4l, 4l + 4) of each half of the run's 2048 elements, so every fp32
        // state load / store instruction of a wave covers 1 KiB of consecutive bytes and every
        // 16-bit one 512 B. (One 16-B parameter pack per lane made each fp32 state access hit
        // every other 16 B of 2 KiB: half-written lines, 15.3 B written per parameter instead
        // of 14 - profiles/round4/README.md section 5.) The last, short run is split the same
        // way with `rows` lanes per half. Scatter and gather stay plain contiguous copies.
        auto eoff = [&](int64_t i, int h) -> int64_t {
          const int64_t run = i / kCommThreads;
          const int64_t l = i - run * kCommThreads;
          const int64_t left = npk - run * kCommThreads;
          const int64_t rows = left < kCommThreads ? left : kCommThreads;
          return run * kCommThreads * EL + h * rows * 4 + l * 4;
        };
        for (int64_t i0 = threadIdx.x; i0 < npk; i0 += U * kCommThreads) {
          Acc8<E> acc[U][2];
          float4 p4[U][2], m4[U][2], v4[U][2];
          bool live[U];
#pragma unroll
          for (int w = 0; w < U; ++w) {
            const int64_t i = i0 + w * kCommThreads;
            live[w] = i < npk;
            if (!live[w]) continue;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int64_t e0 = eoff(i, h);
              Pack16 g[PT];
#pragma unroll
              for (int s = 0; s < PT; ++s) g[s] = ld16_nt(rg, static_cast<uint32_t>(e0 * 4));
#pragma unroll
              for (int s = 0; s < PT; ++s) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[w][h].v[k] += __uint_as_float(g[s][k]);
              }
              p4[w][h] = *reinterpret_cast<const float4*>(sp + e0);
              m4[w][h] = *reinterpret_cast<const float4*>(sm + e0);
              v4[w][h] = *reinterpret_cast<const float4*>(sv + e0);
            }
          }
#pragma unroll
          for (int w = 0; w < U; ++w) {
            if (!live[w]) continue;
            const int64_t i = i0 + w * kCommThreads;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int64_t e0 = eoff(i, h);
              Acc8<E>& ac = acc[w][h];
              ac.v[0] = adamw(ac.v[0] * coef, &p4[w][h].x, &m4[w][h].x, &v4[w][h].x, a);
              ac.v[1] = adamw(ac.v[1] * coef, &p4[w][h].y, &m4[w][h].y, &v4[w][h].y, a);
              ac.v[2] = adamw(ac.v[2] * coef, &p4[w][h].z, &m4[w][h].z, &v4[w][h].z, a);
              ac.v[3] = adamw(ac.v[3] * coef, &p4[w][h].w, &m4[w][h].w, &v4[w][h].w, a);
              *reinterpret_cast<float4*>(sp + e0) = p4[w][h];
              *reinterpret_cast<float4*>(sm + e0) = m4[w][h];
              *reinterpret_cast<float4*>(sv + e0) = v4[w][h];
              const uint2 o = ac.pack(1.f);
              *reinterpret_cast<uint2*>(own_out + e0 * 2) = o;
              typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
              const u32x2 ov = {o.x, o.y};
              for (int k = 0; k < P; ++k)
                if (k != r)
                  __builtin_amdgcn_raw_buffer_store_b64(ov, slab_rsrc(a.base[k] + roff), static_cast<int>(e0 * 2), 0,
                                                        kAuxWt);
            }
          }
        }
      } else
      // U packs per lane per iteration, every load issued before the first use: the
      // persistent grid has only 2 workgroups per CU, so bytes in flight come from ILP
      for (int64_t i0 = threadIdx.x; i0 < npk; i0 += U * kCommThreads) {
        Acc<E> acc[U];
        float4 p4[U][EL / 4], m4[U][EL / 4], v4[U][EL / 4];
        bool live[U];
#pragma unroll
        for (int w = 0; w < U; ++w) {
          const int64_t i = i0 + w * kCommThreads;
          live[w] = i < npk;
          acc[w].zero();
          if (!live[w]) continue;
#pragma unroll
          for (int e = 0; e < EL / 4; ++e) {
            Pack16 g[PT];
#pragma unroll
            for (int s = 0; s < PT; ++s) g[s] = ld16_nt(rg, static_cast<uint32_t>((i * EL + 4 * e) * 4));
#pragma unroll
            for (int s = 0; s < PT; ++s) {
#pragma unroll
              for (int k = 0; k < 4; ++k) acc[w].v[4 * e + k] += __uint_as_float(g[s][k]);
            }
          }
#pragma unroll
          for (int e = 0; e < EL / 4; ++e) {
            p4[w][e] = ld_state<STREAM>(sp, rp, i * EL + 4 * e);
            m4[w][e] = ld_state<STREAM>(sm, rm, i * EL + 4 * e);
            v4[w][e] = ld_state<STREAM>(sv, rv, i * EL + 4 * e);
          }
        }
#pragma unroll
        for (int w = 0; w < U; ++w) {
          if (!live[w]) continue;
          const int64_t i = i0 + w * kCommThreads;
#pragma unroll
          for (int e = 0; e < EL / 4; ++e) {
            acc[w].v[4 * e + 0] = adamw(acc[w].v[4 * e + 0] * coef, &p4[w][e].x, &m4[w][e].x, &v4[w][e].x, a);
            acc[w].v[4 * e + 1] = adamw(acc[w].v[4 * e + 1] * coef, &p4[w][e].y, &m4[w][e].y, &v4[w][e].y, a);
            acc[w].v[4 * e + 2] = adamw(acc[w].v[4 * e + 2] * coef, &p4[w][e].z, &m4[w][e].z, &v4[w][e].z, a);
            acc[w].v[4 * e + 3] = adamw(acc[w].v[4 * e + 3] * coef, &p4[w][e].w, &m4[w][e].w, &v4[w][e].w, a);
            st_state<STREAM>(sp, rp, i * EL + 4 * e, p4[w][e]);
            st_state<STREAM>(sm, rm, i * EL + 4 * e, m4[w][e]);
            st_state<STREAM>(sv, rv, i * EL + 4 * e, v4[w][e]);
          }
          const Pack16 o = acc[w].pack();
          if constexpr (STREAM == 1)
            st16_wt(slab_rsrc(own_out), static_cast<uint32_t>(i * 16), o);
          else
            st16(own_out + i * 16, o);
          for (int k = 0; k < P; ++k)
            if (k != r) st16_wt(slab_rsrc(a.base[k] + roff), static_cast<uint32_t>(i * 16), o);
        }
      }
      const int64_t t = npk * EL + threadIdx.x;
      if (t < len) {
        float g = 0.f;
        for (int s = 0; s < PT; ++s) g += ld_scalar_nt<F32>(rg, t);
        const float pv = adamw(g * coef, sp + t, sm + t, sv + t, a);
        Scalar<E>::store(own_out, t, pv);
        for (int k = 0; k < P; ++k)
          if (k != r) st_scalar_wt<E>(slab_rsrc(a.base[k] + roff), t, pv);
      }
    }
    publish_flags([&](int k) -> uint32_t* { return k == r ? nullptr : f2(a, k, r, u); }, P, epoch, rel);
  }

  // Gather the other owners' updated parameter chunks (phase 3 of the fused step)
  for (int u = blockIdx.x; u < nu; u += G) {
    const int c = u / Pm1;
    const int j = (r + 1 + u % Pm1) % P;
    const int64_t bstart = static_cast<int64_t>(j) * a.block;
    const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
    const int64_t len = clamp_len(clamp_len(a.n - bstart, a.block) - cstart, a.chunk);
    wait_flags([&](int q) -> const uint32_t* { return f2(a, r, j, c * a.sub + q); }, a.sub, epoch, deadline, err,
               ERR_TIMEOUT_REDUCE, acq);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err))
      copy_from_slab<E>(param + (bstart + cstart) * es, a.base[r] + a.off_R + j * slot + cstart * es, len);
  }
  finish_launch_done(a, ctl, epoch, r, kHazR);  // peers may still gather from R
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

void launch_adamw_shard(const CommArgs& a, dim3 grid, hipStream_t s, DType dt) {
  dispatch_dtype(static_cast<int>(dt), [&](auto tag) {
    using E = decltype(tag);
    // 16-bit parameters: run-contiguous halves; fp32: the generic body, plain state access
    if constexpr (E::ELEMS == 8)
      hipLaunchKernelGGL((adamw_shard_kernel<E, 3, 2>), grid, dim3(kCommThreads), 0, s, a);
    else
      hipLaunchKernelGGL((adamw_shard_kernel<E, 0, 2>), grid, dim3(kCommThreads), 0, s, a);
  });
}

}  // namespace mxar
