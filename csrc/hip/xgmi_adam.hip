// Fused sharded-data-parallel step over xGMI (gfx950): reduce-scatter of the gradients,
// AdamW on the owned shard and all-gather of the updated parameters in ONE launch.
//
// The reference hands every reduced vector to a user `dataSink` (AllreduceWorker.scala:
// 180-192); in training that sink is an optimizer. Here the sink runs inside the owner's
// reduce (the allreduce's phase 2): the moment chunk c of the own block has all P gradient
// contributions, the owner sums them (fp32, rank order, x scale), applies AdamW to its fp32
// master copy and moments of that chunk, rounds the new parameters once to the parameter
// dtype and pushes THEM - not the gradient sum - to every peer. Phase 3 gathers the peers'
// updated parameter chunks. Compared with reduce-scatter + optimizer + all-gather this saves
// two launches, the round trip of the reduced gradient through HBM and the serialisation
// between the three steps; the wire bytes are those of one allreduce.
//
// Slot reuse across launches is the two-shot's: a rank finishes a launch only after it has
// received every owner's updated chunk, which each owner sends after reading its S slot for
// that chunk; peers' pending reads of R are covered by entry_guard / finish_launch_done.
#include "../core/env.h"
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "xgmi_adam_device.h"

namespace mxar {

template <class E, int PT, int STREAM, int U>
__global__ __launch_bounds__(kCommThreads) void twoshot_adamw_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  const StepCtx k(a, PT > 0 ? PT : a.P);
  const int y = blockIdx.y;
  const int r = k.r;
  const char* const grad = a.in[y];
  // The slot stride is read here, once, not where RedSrc is formed in the unit loop: with
  // a.slot_bytes there the compiler (AMD clang 22.0.0git, ROCm 7.2.0) reserved a 36-byte scratch
  // frame that no instruction used, in twelve instantiations. Only the resource remarks show it,
  // nothing tests it: profiles/shard_step_refactor.md.
  const int64_t slot = a.slot_bytes;

  // Phase 1 - gradient ScatterBlock: chunk c of block j to its owner j
  if (static_cast<int>(blockIdx.x) < k.nu) entry_guard(a, k.ctl, r, k.epoch, kHazS, -1, k.deadline, k.err);
  scatter_grads<E>(a, k, grad);

  // Phase 2 - reduce own chunk, AdamW on the owned shard, push the new parameters
  const int64_t bstart_own = static_cast<int64_t>(r) * a.block;
  const int nu2 = a.nch * a.sub;
  for (int u = blockIdx.x; u < nu2; u += k.G) {
    const OwnUnit o = own_unit(a, r, u);
    wait_flags([&](int s) -> const uint32_t* { return s == r ? nullptr : f1(a, r, s, o.c); }, k.P, k.epoch, k.deadline,
               k.err, ERR_TIMEOUT_SCATTER, k.acq);
    if (o.len > 0 && unit_in_bounds(a, o.cstart * es, o.len * es, u, k.err)) {
      const RedSrc src{grad + (bstart_own + o.cstart) * es, a.base[r] + a.off_S + o.cstart * es, slot, r};
      adamw_unit<E, STREAM, U>(a, k.P, r, o.cstart, o.len, PeerSumGrad<E, PT>{src, k.P, a.scale});
    }
    publish_flags([&](int p) -> uint32_t* { return p == r ? nullptr : f2(a, p, r, u); }, k.P, k.epoch, k.rel);
  }

  // Phase 3 - gather the other owners' updated parameter chunks
  gather_params<E>(a, k, a.out[y]);
  finish_launch_done(a, k.ctl, k.epoch, r, kHazR);  // peers may still gather from R
}

template <int STREAM, int U>
static void launch_adamw_t(const CommArgs& a, dim3 grid, hipStream_t s, DType dt) {
  dispatch_dtype(static_cast<int>(dt), [&](auto tag) {
    using E = decltype(tag);
    // P is a template constant wherever it can be: the reduce then issues every source's
    // load before the first add (the PT = 0 loop waits on each load in turn) - P = 1 is the
    // single-GPU optimizer step
    switch (a.P) {
      case 1: hipLaunchKernelGGL((twoshot_adamw_kernel<E, 1, STREAM, U>), grid, dim3(kCommThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL((twoshot_adamw_kernel<E, 2, STREAM, U>), grid, dim3(kCommThreads), 0, s, a); break;
      case 4: hipLaunchKernelGGL((twoshot_adamw_kernel<E, 4, STREAM, U>), grid, dim3(kCommThreads), 0, s, a); break;
      case 8: hipLaunchKernelGGL((twoshot_adamw_kernel<E, 8, STREAM, U>), grid, dim3(kCommThreads), 0, s, a); break;
      default: hipLaunchKernelGGL((twoshot_adamw_kernel<E, 0, STREAM, U>), grid, dim3(kCommThreads), 0, s, a); break;
    }
  });
}

void launch_adamw(const CommArgs& a, dim3 grid, hipStream_t s, DType dt) {
  // study knob MXAR_ADAM_STREAM (state access form, above); two packs per lane in flight (1
  // and 4 measured no better - their knob was removed in round 6)
  static const int mode = [] {
    const char* e = study_env("MXAR_ADAM_STREAM");
    return e != nullptr ? std::atoi(e) : -1;
  }();
  if (mode == 3 || (mode < 0 && dt != DType::F32))
    launch_adamw_t<3, 2>(a, grid, s, dt);  // 16-bit parameters: run-contiguous halves (default)
  else if (mode == 1)
    launch_adamw_t<1, 2>(a, grid, s, dt);
  else if (mode == 2)
    launch_adamw_t<2, 2>(a, grid, s, dt);
  else
    launch_adamw_t<0, 2>(a, grid, s, dt);
}

}  // namespace mxar
