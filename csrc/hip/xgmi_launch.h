// Host entries of the data-plane kernels: each `.hip` file keeps its kernels and one launcher
// per kernel family; XgmiComm (xgmi_comm.cc, host C++) fills CommArgs and calls them.
#pragma once

#include <hip/hip_runtime_api.h>

#include "comm_args.h"
#include "xgmi_comm.h"

namespace mxar {

// Two-shot / one-shot / ring (fp32 or element-type partials) allreduce (xgmi_comm.hip).
void launch_allreduce(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, Algo kind);
// Device-side barrier over all ranks: dim3(1, ranks in the launch) (xgmi_comm.hip).
void launch_barrier(const CommArgs& a, dim3 grid, hipStream_t s);
// Host entry of the threshold kernel (xgmi_threshold.hip).
void launch_threshold(const CommArgs& a, dim3 grid, hipStream_t s, DType dt);
// A plane group's resident kernel: dim3(grid, workers + 1) (xgmi_threshold.hip).
void launch_threshold_group_resident(const CommArgs& a, const GroupResArgs& g, int grid, hipStream_t s, DType dt);
// Resident rounds (xgmi_threshold.hip; XgmiComm::launch_resident).
void launch_threshold_resident(const CommArgs& a, int grid, hipStream_t s, DType dt, const ResidentDoor* door,
                               uint32_t* hstate, uint32_t* dm, uint32_t seq, uint32_t gen, uint64_t idle_ticks);
// Progress words = value in every peer's slab (xgmi_threshold.hip; XgmiComm::publish_progress).
void launch_publish_progress(const CommArgs& a, uint32_t value, hipStream_t s);
// Host entry of the low-latency one-shot (xgmi_ll.hip).
void launch_ll(const CommArgs& a, dim3 grid, hipStream_t s, DType dt);
// Host entry of the fused reduce-scatter + AdamW + all-gather (xgmi_adam.hip).
void launch_adamw(const CommArgs& a, dim3 grid, hipStream_t s, DType dt);
// Host entries of the clipped step's two halves (xgmi_clip.hip): reduce-scatter into the fp32
// shard with the sum of squares; AdamW from the shard times the clip coefficient + all-gather.
// accumulate: gshard += the scaled sum (fp32, product rounded before the add) instead of =
void launch_rs_sq(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, bool accumulate);
// record: a.coef[y] points at a StepRecord (coefficient, skip word, bias corrections)
void launch_adamw_shard(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, bool record = false);
// Host entry of the loss-scaled step's one-wave control kernel (xgmi_scale.hip).
void launch_scale_step(const ScaleStepArgs& a, hipStream_t s);
// Host entry of all-to-all (mode 0) / all-gather (1) / reduce-scatter (2) (xgmi_coll.hip).
void launch_coll(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, int mode);
// Host entry of the rooted broadcast / reduce, root = a.root (xgmi_rooted.hip).
void launch_rooted(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, Rooted kind);

}  // namespace mxar
