// Step control of the loss-scaled sharded-data-parallel step (gfx950): one wave, launched on the
// stream between the two halves of the split step (xgmi_clip.hip), after the ranks' 16-byte
// sum-of-squares records were all-gathered. It decides on the device what the host would need a
// sync to know - whether some reduced gradient element was non-finite - and leaves that decision,
// the coefficient and AdamW's bias corrections in a StepRecord (comm_args.h) for the update
// halves of every bucket. No host sync, no floating-point atomics, nothing shared between ranks:
// every rank runs it on its own copy of the same records and gets the same bits.
//
// The rule is parallel/loss_scale.py `scale_step_rule`, plain torch ops; this kernel gives its
// bits (tests/test_loss_scale_gpu.py holds them against each other on finite, inf and NaN totals):
//
//   total = recs[0][0] + recs[1][0] + ...        float64, rank order
//   found = !isfinite(total)
//   inv   = 1 / S                                fp32, S the scale before this step
//   norm  = fl32(sqrt64(total)) * inv
//   clip  = min(1, fl32(1 / fl32(norm + 1e-6f)) * max_norm), 1.0f when not clipping
//           (torch evaluates `max_norm / x` on a tensor x as reciprocal(x) * max_norm: two
//           roundings, and clip_coef_from_records has always given these bits)
//   coef  = clip * inv
//   found:  S *= backoff, tracker = 0, skipped += 1
//   else:   tracker += 1; tracker == interval: S *= growth, tracker = 0; applied += 1
//   (a static scale and its tracker never change)
//
// Divide and square root are IEEE (the compiler's default for HIP, and the kernels of the step
// already rest on it). Where the rule rounds twice the kernel must not contract: norm is pinned
// as an fp32 register value before 1e-6f is added (else fma(sqrt, inv, 1e-6f)), with the empty
// asm of adamw() (xgmi_adam_device.h). A NaN's payload and sign are the one thing left open:
// IEEE does not fix them, the host's and the device's differ, and nothing reads them.
//
// Bias corrections: c1 = 1 - beta1^t and c2_sqrt = sqrt(1 - beta2^t) are computed on the host
// in fp32 with std::pow (set_adamw_hyper, xgmi_comm.cc) in every other step of this project, and
// the device's powf need not round alike. So they are not computed here: the host keeps a table
// of its own values, filled ahead of the largest count the next step can reach, and this kernel
// copies the entry of `applied` after its increment. The table ends at the first count where
// both are exactly 1.0f, and the index clamps there. A loss-scaled run therefore applies at count
// t exactly what a plain run applies at step t.
#include <hip/hip_runtime.h>

#include "comm_args.h"
#include "xgmi_launch.h"

namespace mxar {

__global__ __launch_bounds__(64) void scale_step_kernel(ScaleStepArgs a) {
  if (threadIdx.x != 0) return;  // one lane: P additions in rank order and a dozen scalar operations
  double total = a.recs[0];
  for (int k = 1; k < a.P; ++k) total += a.recs[2 * k];
  const bool found = !(__builtin_fabs(total) < __builtin_inf());  // inf or NaN
  ScaleState st = *a.state;
  const float inv = 1.f / st.scale;
  float norm = static_cast<float>(__builtin_sqrt(total)) * inv;
  asm("" : "+v"(norm));  // fl32(sqrt * inv) first: no fma with the 1e-6f below
  float clip = 1.f;
  if (a.clip) {
    float t = norm + 1e-6f;
    asm("" : "+v"(t));
    float rcp = 1.f / t;
    asm("" : "+v"(rcp));
    clip = rcp * a.max_norm;
    asm("" : "+v"(clip));
    clip = clip > 1.f ? 1.f : clip;  // NaN stays NaN, as torch's clamp(max=1) leaves it
  }
  const float coef = clip * inv;

  if (found) {
    ++st.skipped;
    if (a.dynamic) {
      st.scale *= a.backoff;
      st.tracker = 0;
    }
  } else {
    ++st.applied;
    if (a.dynamic && ++st.tracker == a.interval) {
      st.scale *= a.growth;
      st.tracker = 0;
    }
  }
  *a.state = st;

  StepRecord rec;
  rec.coef = coef;
  rec.skip = found ? 1u : 0u;
  rec.norm = norm;
  rec.clip = clip;
  rec.c1 = 1.f;
  rec.c2_sqrt = 1.f;
  rec.short_table = 0u;
  rec.pad = 0u;
  if (!found) {
    int t = st.applied < a.end ? st.applied : a.end;  // past `end` both stay 1.0f
    if (t > a.filled) {  // never, while the host fills ahead: stay inside the table and say so
      t = a.filled;
      rec.short_table = 1u;
    }
    if (t >= 1) {
      rec.c1 = a.table[2 * (t - 1)];
      rec.c2_sqrt = a.table[2 * (t - 1) + 1];
    }
  }
  *a.rec = rec;
}

void launch_scale_step(const ScaleStepArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(scale_step_kernel, dim3(1), dim3(64), 0, s, a);
}

}  // namespace mxar
