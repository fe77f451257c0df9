// Device code shared by the two kernels that run AdamW on a rank's shard: the fused step
// (xgmi_adam.hip: the gradient is the P-way sum of the scattered chunks) and the update half of
// the clipped step (xgmi_clip.hip: the gradient is the fp32 shard the reduce-scatter half left,
// times the clip coefficient). One copy of adamw() and of the fp32 state access forms.
#pragma once

#include "xgmi_device.h"

namespace mxar {

// AdamW (decoupled weight decay, PyTorch semantics) of one element; returns the new param.
__device__ __forceinline__ float adamw(float g, float* p, float* m, float* v, const CommArgs& a) {
  float pv = *p;
  pv *= 1.f - a.lr * a.wd;
  const float mv = a.beta1 * *m + (1.f - a.beta1) * g;
  const float vv = a.beta2 * *v + (1.f - a.beta2) * g * g;
  const float denom = sqrtf(vv) / a.c2_sqrt + a.eps;
  pv -= (a.lr / a.c1) * mv / denom;
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

// fp32 state access: plain loads / stores (STREAM = false, the default) or nt loads +
// write-through stores (STREAM = true, MXAR_ADAM_STREAM=1: the store probe's fastest copy
// form, profiles/round3/store_probe.json). The state is read and written back at the same
// addresses, and the streaming form is 1.56x slower (1.00 vs 0.64 ms for the 134 M-parameter
// step, same box: profiles/round3/adamw_stream_ab.jsonl); the gradients (read once, summed)
// come in with nt loads either way.
// MODE 0 (default): plain state loads and stores. MODE 1 (MXAR_ADAM_STREAM=1): nt loads +
// write-through stores (the store probe's fastest copy form, profiles/round3/store_probe.json)
// - the state is read and written back at the same addresses, and that form was 1.56x slower
// (1.00 vs 0.64 ms for the 134 M-parameter step, same box: profiles/round3/README.md).
// MODE 2 (MXAR_ADAM_STREAM=2): nt loads, plain stores. The gradients (read once, summed) come
// in with nt loads in every mode.
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

}  // namespace mxar
