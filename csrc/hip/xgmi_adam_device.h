// Device code shared by the kernels of the sharded-data-parallel step: the fused step
// (xgmi_adam.hip, twoshot_adamw_kernel) and the two halves of the clipped step (xgmi_clip.hip,
// rs_sq_kernel and adamw_shard_kernel). One copy each of the launch prologue, the unit geometry,
// the gradient scatter and parameter gather phases, adamw(), the fp32 state access forms and the
// AdamW update of one reduce unit, which takes its gradient from one of two sources: the P-way
// sum of the scattered chunks (fused step) or the fp32 shard the reduce-scatter half left, times
// the clip coefficient (update half; in a loss-scaled step with coefficient and bias corrections
// from the step record, RecordGrad).
#pragma once

#include "xgmi_device.h"

namespace mxar {

// What every kernel of the step derives from its arguments before its first phase.
struct StepCtx {
  int P, r, G;  // ranks, this rank, workgroups per rank
  uint32_t* ctl;
  uint32_t epoch;
  uint64_t deadline;
  uint32_t* err;
  bool rel, acq;
  int Pm1, nu;  // peers (at least 1: a divisor), scatter / gather units
  __device__ __forceinline__ StepCtx(const CommArgs& a, int P_)
      : P(P_), r(a.rank0 + blockIdx.y), G(gridDim.x), ctl(a.ctl[blockIdx.y]), epoch(launch_epoch(ctl)),
        deadline(wall_ticks() + a.timeout), err(&ctl[2]), rel(a.fence & 1), acq(a.fence & 2),
        Pm1(P_ > 1 ? P_ - 1 : 1), nu((P_ - 1) * a.nch) {}
};

// Reduce unit u of the own block: sub-unit u % sub of chunk c = u / sub. cstart in elements
// from the block's start; len = 0 past the block's valid length.
struct OwnUnit {
  int c;
  int64_t cstart, len;
};
__device__ __forceinline__ OwnUnit own_unit(const CommArgs& a, int r, int u) {
  const int c = u / a.sub;
  const int64_t cbeg = static_cast<int64_t>(c) * a.chunk;
  const int64_t qbeg = static_cast<int64_t>(u % a.sub) * a.subchunk;
  const int64_t blen = clamp_len(a.n - static_cast<int64_t>(r) * a.block, a.block);
  return {c, cbeg + qbeg, clamp_len(clamp_len(blen - cbeg, a.chunk) - qbeg, a.subchunk)};
}

// Scatter / gather unit u: chunk c of peer j's block, the peers taken in the order r + 1, ...
struct PeerUnit {
  int c, j;
  int64_t bstart, cstart, len;
};
__device__ __forceinline__ PeerUnit peer_unit(const CommArgs& a, const StepCtx& k, int u) {
  const int c = u / k.Pm1;
  const int j = (k.r + 1 + u % k.Pm1) % k.P;
  const int64_t bstart = static_cast<int64_t>(j) * a.block;
  const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
  return {c, j, bstart, cstart, clamp_len(clamp_len(a.n - bstart, a.block) - cstart, a.chunk)};
}

// Gradient ScatterBlock: chunk c of block j to its owner j. The caller took the entry guard.
template <class E>
__device__ __forceinline__ void scatter_grads(const CommArgs& a, const StepCtx& k, const char* grad) {
  constexpr int es = 16 / E::ELEMS;
  for (int u = blockIdx.x; u < k.nu; u += k.G) {
    const PeerUnit p = peer_unit(a, k, u);
    if (p.len > 0 && unit_in_bounds(a, p.cstart * es, p.len * es, p.c, k.err))
      copy_to_slab<E>(a.base[p.j] + a.off_S + k.r * a.slot_bytes + p.cstart * es, grad + (p.bstart + p.cstart) * es,
                      p.len);
    publish_flags([&](int) { return f1(a, p.j, k.r, p.c); }, 1, k.epoch, k.rel);
  }
}

// Gather the other owners' updated parameter chunks, each once all its sub-units are in.
template <class E>
__device__ __forceinline__ void gather_params(const CommArgs& a, const StepCtx& k, char* param) {
  constexpr int es = 16 / E::ELEMS;
  for (int u = blockIdx.x; u < k.nu; u += k.G) {
    const PeerUnit p = peer_unit(a, k, u);
    wait_flags([&](int q) -> const uint32_t* { return f2(a, k.r, p.j, p.c * a.sub + q); }, a.sub, k.epoch, k.deadline,
               k.err, ERR_TIMEOUT_REDUCE, k.acq);
    if (p.len > 0 && unit_in_bounds(a, p.cstart * es, p.len * es, p.c, k.err))
      copy_from_slab<E>(param + (p.bstart + p.cstart) * es, a.base[k.r] + a.off_R + p.j * a.slot_bytes + p.cstart * es,
                        p.len);
  }
}

// One moment update b * s + c * g with its roundings fixed: one product is rounded to fp32 (the
// empty asm pins it as a register value, so it cannot be contracted), the other goes into the
// fma unrounded. Written as a sum of two products the choice is the compiler's - it orders the
// operands of the add by where their loads sit and contracts the first - and it came out
// differently by element position and by kernel (profiles/shard_step_refactor.md).
// gf: fma(c, g, fl(b * s)); otherwise fma(b, s, fl(c * g)). gf is a constant at every call
// once the callers' loops are unrolled.
__device__ __forceinline__ float moment(bool gf, float b, float s, float c, float g) {
  float t = gf ? b * s : c * g;
  asm("" : "+v"(t));
  return gf ? __builtin_fmaf(c, g, t) : __builtin_fmaf(b, s, t);
}

// Which product of the moment updates is rounded, by the element's place in adamw_unit: pack w
// of the lane's U, element k of the float4. The state's product is the rounded one, except in
// elements x and y of the second pack under plain state loads and in the scalar tail. The rule
// has NO numerical merit: it is what a compiler once happened to choose while the choice was
// still its own, and it is kept only so that a run gives the bits of earlier builds (checkpoints
// and reruns compare equal; `tools/clip_step_cost.py --digest` against such a build is what
// checks that - the test of this rule checks only that the kernels follow it). When a change of
// numerics is decided, it may go: one order for every element would do as well.
template <int STREAM>
constexpr bool grad_fused(int w, int k) {
  return !((STREAM == 0 || STREAM == 3) && w == 1 && k < 2);
}

// AdamW's bias corrections of one launch: c1 = 1 - beta1^t, c2_sqrt = sqrt(1 - beta2^t). The
// gradient source says where they come from (its corr()): the launch arguments, where the host
// put them for its own step count, or the step record of a loss-scaled step, where the control
// kernel put the host's values for the device's count (xgmi_scale.hip).
struct BiasCorr {
  float c1, c2_sqrt;
};

// AdamW (decoupled weight decay, PyTorch semantics) of one element; returns the new param.
__device__ __forceinline__ float adamw(bool gf, float g, float* p, float* m, float* v, const CommArgs& a,
                                       const BiasCorr& bc) {
  float pv = *p;
  pv *= 1.f - a.lr * a.wd;
  const float mv = moment(gf, a.beta1, *m, 1.f - a.beta1, g);
  const float vv = moment(gf, a.beta2, *v, (1.f - a.beta2) * g, g);
  const float denom = sqrtf(vv) / bc.c2_sqrt + a.eps;
  pv -= (a.lr / bc.c1) * mv / denom;
  // The callers round the returned value to the parameter dtype: it must be the fp32 value the
  // master holds. Left to itself the compiler folds the last multiply-subtract and the fp16
  // conversion of the scalar tail into one v_fma_mixlo_f16, which rounds the unrounded result
  // straight to fp16 - at a tie of the fp32 value a parameter one fp16 ulp off master.to(fp16)
  // (tests/test_adamw_gpu.py). The empty asm pins pv as an fp32 register value; no instruction.
  asm("" : "+v"(pv));
  *p = pv;
  *m = mv;
  *v = vv;
  return pv;
}

// fp32 state access. MODE 0 (default): plain state loads and stores. MODE 1
// (MXAR_ADAM_STREAM=1): nt loads + write-through stores (the store probe's fastest copy form,
// profiles/round3/store_probe.json) - the state is read and written back at the same addresses,
// and that form was 1.56x slower (1.00 vs 0.64 ms for the 134 M-parameter step, same box:
// profiles/round3/adamw_stream_ab.jsonl). MODE 2 (MXAR_ADAM_STREAM=2): nt loads, plain stores.
// The gradients (read once, summed) come in with nt loads in every mode.
template <int MODE>
__device__ __forceinline__ float4 ld_state(const float* p, __amdgpu_buffer_rsrc_t r, int64_t i) {
  if constexpr (MODE != 0) {
    const Pack16 v = ld16_nt(r, static_cast<uint32_t>(i * 4));
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
  } else {
    return *reinterpret_cast<const float4*>(p + i);
  }
}
template <int MODE>
__device__ __forceinline__ void st_state(float* p, __amdgpu_buffer_rsrc_t r, int64_t i, const float4& x) {
  if constexpr (MODE == 1) {
    Pack16 v;
    v[0] = __float_as_uint(x.x);
    v[1] = __float_as_uint(x.y);
    v[2] = __float_as_uint(x.z);
    v[3] = __float_as_uint(x.w);
    st16_wt(r, static_cast<uint32_t>(i * 4), v);
  } else {
    *reinterpret_cast<float4*>(p + i) = x;
  }
}

// Gradient sources of adamw_unit. Each adds the fp32 gradient of pack i (16 B of parameters),
// of the 4 elements from e0 (run-contiguous halves) or of tail element t into a zeroed
// accumulator; adamw() gets that sum times `mul`.
//
// The fused step: the sum of P contributions in rank order, mul = scale. P is a template
// constant wherever it can be: every source's load then issues before the first add (the
// PT = 0 loop waits on each load in turn).
template <class E, int PT>
struct PeerSumGrad {
  RedSrc src;
  int P;
  float mul;
  __device__ __forceinline__ void add_pack(Acc<E>& acc, int64_t i) const {
    if constexpr (PT > 0) {
      Pack16 g[PT];
#pragma unroll
      for (int s = 0; s < PT; ++s) g[s] = ld16_nt(src.rsrc(s), static_cast<uint32_t>(i * 16));
#pragma unroll
      for (int s = 0; s < PT; ++s) acc.add(g[s]);
    } else {
      for (int s = 0; s < P; ++s) acc.add(ld16_nt(src.rsrc(s), static_cast<uint32_t>(i * 16)));
    }
  }
  __device__ __forceinline__ void add_half(Acc8<E>& acc, int64_t e0) const {
    if constexpr (PT > 0) {
      uint2 g[PT];
#pragma unroll
      for (int s = 0; s < PT; ++s) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(src.rsrc(s), static_cast<int>(e0 * 2), 0, kAuxNt);
        g[s] = make_uint2(v[0], v[1]);
      }
#pragma unroll
      for (int s = 0; s < PT; ++s) acc.add(g[s]);
    } else {
      for (int s = 0; s < P; ++s) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(src.rsrc(s), static_cast<int>(e0 * 2), 0, kAuxNt);
        acc.add(make_uint2(v[0], v[1]));
      }
    }
  }
  __device__ __forceinline__ float tail(int64_t t) const {
    float g = 0.f;
    for (int s = 0; s < P; ++s) g += ld_scalar_nt<E>(src.rsrc(s), t);
    return g;
  }
  __device__ __forceinline__ BiasCorr corr(const CommArgs& a) const { return {a.c1, a.c2_sqrt}; }
};

// The update half of the clipped step: the unit's fp32 shard, read once (nt loads), mul = the
// clip coefficient.
template <class E>
struct ShardGrad {
  __amdgpu_buffer_rsrc_t rg;
  float mul;
  __device__ __forceinline__ void add4(float* v, int64_t e0) const {
    const Pack16 g = ld16_nt(rg, static_cast<uint32_t>(e0 * 4));
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += __uint_as_float(g[k]);
  }
  __device__ __forceinline__ void add_pack(Acc<E>& acc, int64_t i) const {
#pragma unroll
    for (int e = 0; e < E::ELEMS / 4; ++e) add4(acc.v + 4 * e, i * E::ELEMS + 4 * e);
  }
  __device__ __forceinline__ void add_half(Acc8<E>& acc, int64_t e0) const { add4(acc.v, e0); }
  __device__ __forceinline__ float tail(int64_t t) const { return 0.f + ld_scalar_nt<F32>(rg, t); }
  __device__ __forceinline__ BiasCorr corr(const CommArgs& a) const { return {a.c1, a.c2_sqrt}; }
};

// The update half of a loss-scaled step: the same shard, mul = the step record's coefficient
// (clip / scale) and the corrections the record carries.
template <class E>
struct RecordGrad : ShardGrad<E> {
  BiasCorr bc;
  __device__ __forceinline__ RecordGrad(__amdgpu_buffer_rsrc_t rg_, const StepRecord& rec)
      : ShardGrad<E>{rg_, rec.coef}, bc{rec.c1, rec.c2_sqrt} {}
  __device__ __forceinline__ BiasCorr corr(const CommArgs&) const { return bc; }
};

// AdamW on `len` elements from `cstart` of rank r's shard (one reduce unit, one workgroup): the
// gradient from `grad`, the fp32 master copy and moments updated in place, the new parameters
// rounded once to the parameter dtype, stored to the own output and pushed write-through into
// every peer's R slot.
template <class E, int STREAM, int U, class Grad>
__device__ __forceinline__ void adamw_unit(const CommArgs& a, int P, int r, int64_t cstart, int64_t len,
                                           const Grad grad) {
  constexpr int es = 16 / E::ELEMS;
  constexpr int EL = E::ELEMS;
  const int y = blockIdx.y;
  char* own_out = a.out[y] + (static_cast<int64_t>(r) * a.block + cstart) * es;
  const int64_t roff = a.off_R + r * a.slot_bytes + cstart * es;
  float* const sp = a.opt_p[y] + cstart;
  float* const sm = a.opt_m[y] + cstart;
  float* const sv = a.opt_v[y] + cstart;
  const __amdgpu_buffer_rsrc_t rp = slab_rsrc(sp), rm = slab_rsrc(sm), rv = slab_rsrc(sv);
  const int64_t npk = len / EL;
  const BiasCorr bc = grad.corr(a);
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
          grad.add_half(acc[w][h], e0);
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
          ac.v[0] = adamw(grad_fused<STREAM>(w, 0), ac.v[0] * grad.mul, &p4[w][h].x, &m4[w][h].x, &v4[w][h].x, a, bc);
          ac.v[1] = adamw(grad_fused<STREAM>(w, 1), ac.v[1] * grad.mul, &p4[w][h].y, &m4[w][h].y, &v4[w][h].y, a, bc);
          ac.v[2] = adamw(grad_fused<STREAM>(w, 2), ac.v[2] * grad.mul, &p4[w][h].z, &m4[w][h].z, &v4[w][h].z, a, bc);
          ac.v[3] = adamw(grad_fused<STREAM>(w, 3), ac.v[3] * grad.mul, &p4[w][h].w, &m4[w][h].w, &v4[w][h].w, a, bc);
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
  } else {
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
        grad.add_pack(acc[w], i);
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
          float* const g = acc[w].v + 4 * e;
          g[0] = adamw(grad_fused<STREAM>(w, 0), g[0] * grad.mul, &p4[w][e].x, &m4[w][e].x, &v4[w][e].x, a, bc);
          g[1] = adamw(grad_fused<STREAM>(w, 1), g[1] * grad.mul, &p4[w][e].y, &m4[w][e].y, &v4[w][e].y, a, bc);
          g[2] = adamw(grad_fused<STREAM>(w, 2), g[2] * grad.mul, &p4[w][e].z, &m4[w][e].z, &v4[w][e].z, a, bc);
          g[3] = adamw(grad_fused<STREAM>(w, 3), g[3] * grad.mul, &p4[w][e].w, &m4[w][e].w, &v4[w][e].w, a, bc);
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
  }
  const int64_t t = npk * EL + threadIdx.x;
  if (t < len) {
    const float pv = adamw(false, grad.tail(t) * grad.mul, sp + t, sm + t, sv + t, a, bc);
    Scalar<E>::store(own_out, t, pv);
    for (int k = 0; k < P; ++k)
      if (k != r) st_scalar_wt<E>(slab_rsrc(a.base[k] + roff), t, pv);
  }
}

}  // namespace mxar
