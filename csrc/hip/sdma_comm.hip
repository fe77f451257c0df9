// SdmaComm's device side (host side: sdma_comm.cc; schedule: csrc/runtime/sdma_schedule.h):
// the signal release, and the small-grid pipelined reduce and gather kernels with their
// bounded flag waits.
#include <hip/hip_runtime.h>

#include "sdma_launch.h"
#include "xgmi_device.h"

namespace mxar {

namespace {
__host__ __device__ inline int64_t rup(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace

__global__ void sdma_release_kernel(int64_t* sig) {
  if (threadIdx.x == 0) __hip_atomic_store(sig, int64_t{0}, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ int64_t sdma_blen(const SdmaLaunch& L, int s) {
  return sdma_block_len(L.n, L.block, s);
}

// Own block = scale x (own input + the P-1 SD slots), fixed order s = 0..P-1, fp32, written
// through (the engines read it from memory for phase 2), piece by piece: piece k is reduced
// once every peer's FS[s][k] shows the epoch, and its last workgroup releases mid[k] - the
// signal the engines' phase-2 copies of piece k wait on. No workgroup waits for another.
template <class E>
__global__ __launch_bounds__(kCommThreads) void sdma_reduce_kernel(SdmaLaunch L) {
  constexpr int es = 16 / E::ELEMS;
  const SdmaRankArgs& a = L.y[blockIdx.y];
  const int G = static_cast<int>(gridDim.x);
  const uint64_t deadline = wall_ticks() + L.timeout;
  const int64_t rl = sdma_blen(L, a.r);
  const int64_t own0 = static_cast<int64_t>(a.r) * L.block;
  for (int k = 0; k < L.K; ++k) {
    const int64_t p0 = static_cast<int64_t>(k) * L.pe;
    const int64_t lk = clamp_len(rl - p0, L.pe);
    if (lk <= 0) break;  // uniform
    wait_flags([&](int s) -> const uint32_t* { return s == a.r ? nullptr : a.flags + sdma_fs_word(s, k); }, L.W,
               a.epoch, deadline, a.err, ERR_TIMEOUT_SCATTER);
    const int64_t sub = rup(cdiv(lk, G), E::ELEMS);
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * sub;
    const int64_t l = clamp_len(lk - b0, sub);
    if (l > 0) {
      const RedSrc src{a.in + (own0 + p0 + b0) * es, a.sd + (p0 + b0) * es, L.slot, a.r};
      char* dst = a.out + (own0 + p0 + b0) * es;
      reduce_to<E, 0>(L.W, src, 1, 0, [&](int) -> char* { return dst; }, l, L.scale, true);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: the engines read the piece
      const uint32_t t = __hip_atomic_fetch_add(&a.cnt[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t == static_cast<uint32_t>(G - 1)) {
        __hip_atomic_store(&a.cnt[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.mid[k], int64_t{0}, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// out[block s, piece k] = RD slot s piece k for every s != r, piece by piece as the FR[s][k]
// flags arrive (and the own FR[r][k]: the engines have finished READING the own block's
// piece k for phase 2, so the call is complete for the stream). Plain-memory consumers
// follow on this stream: the stores go through to memory.
template <class E>
__global__ __launch_bounds__(kCommThreads) void sdma_gather_kernel(SdmaLaunch L) {
  constexpr int es = 16 / E::ELEMS;
  const SdmaRankArgs& a = L.y[blockIdx.y];
  const int G = static_cast<int>(gridDim.x);
  const uint64_t deadline = wall_ticks() + L.timeout;
  for (int k = 0; k < L.K; ++k) {
    const int64_t p0 = static_cast<int64_t>(k) * L.pe;
    if (p0 >= L.block) break;  // uniform
    wait_flags([&](int s) -> const uint32_t* {
                 return sdma_blen(L, s) > p0 ? a.flags + sdma_fr_word(s, k) : nullptr;
               },
               L.W, a.epoch, deadline, a.err, ERR_TIMEOUT_REDUCE);
    const int64_t sub = rup(cdiv(L.pe, G), E::ELEMS);
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * sub;
    for (int s = 0; s < L.W; ++s) {
      if (s == a.r) continue;
      const int64_t l = clamp_len(clamp_len(sdma_blen(L, s) - p0, L.pe) - b0, sub);
      if (l > 0)
        copy_from_slab<E>(a.out + (static_cast<int64_t>(s) * L.block + p0 + b0) * es,
                          a.rd + s * L.slot + (p0 + b0) * es, l);
    }
  }
}

void launch_sdma_release(int64_t* sig, hipStream_t s) {
  hipLaunchKernelGGL(sdma_release_kernel, dim3(1), dim3(64), 0, s, sig);
}

void launch_sdma_reduce_gather(const SdmaLaunch& L, int grid, int ny, hipStream_t s, DType dt) {
  dispatch_dtype(static_cast<int>(dt), [&](auto tag) {
    using E = decltype(tag);
    hipLaunchKernelGGL(sdma_reduce_kernel<E>, dim3(grid, ny), dim3(kCommThreads), 0, s, L);
    if (L.W > 1)  // one rank: the reduce wrote the whole (scaled) output
      hipLaunchKernelGGL(sdma_gather_kernel<E>, dim3(grid, ny), dim3(kCommThreads), 0, s, L);
  });
}

}  // namespace mxar
