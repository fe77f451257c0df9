// Rooted collectives over xGMI (gfx950): broadcast and reduce, one launch per segment.
//
// A root that pushed all n bytes to each of its P-1 peers would load every link with n. Both
// kernels use the reference worker's two phases (xgmi_coll.hip) instead, so that every link
// carries about 2n/P:
//   broadcast : the root scatters block j to rank j (S slots) and its own block to everybody
//               (R slots); rank j forwards block j to the other non-roots (R slots) - a
//               scatter, then an all-gather
//   reduce    : every rank pushes block j to rank j (S slots), rank j reduces it (reduce_to:
//               fp32, rank order, one rounding) straight into the root's R slot [j], and the
//               root copies the P-1 reduced blocks out - a reduce-scatter, then a gather
// The tensor is [P] blocks of a.block elements, a.n elements in all: trailing blocks are short
// or empty, and their flags are still published. Flag rows belong to their writer: f1(k, s, c)
// and f2(k, s, c) are only ever written by rank s.
// Launch-sequence invariant (xgmi_device.h entry_guard, xgmi_ll.hip): no rank completes launch
// e before it saw an epoch-e flag from every peer. The reduce waits for every peer's block; a
// broadcast's non-roots wait for every peer's forward; its root would wait for nobody, so each
// non-root acknowledges its entry in f2(root, j, 0) (no payload) and the root waits for those.
#include <hip/hip_runtime.h>

#include "xgmi_device.h"

namespace mxar {

namespace {

// elements of chunk c in block j of a tensor of a.n elements
__device__ __forceinline__ int64_t chunk_len(const CommArgs& a, int j, int c) {
  const int64_t blen = clamp_len(a.n - static_cast<int64_t>(j) * a.block, a.block);
  return clamp_len(blen - static_cast<int64_t>(c) * a.chunk, a.chunk);
}

}  // namespace

// On the root in[y] is the tensor, on the others out[y] (in place).
template <class E>
__global__ __launch_bounds__(kCommThreads) void broadcast_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  const int P = a.P;
  const int y = blockIdx.y;
  const int r = a.rank0 + y;
  const int root = a.root;
  uint32_t* const ctl = a.ctl[y];
  uint32_t* const err = &ctl[2];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  const int G = gridDim.x;
  const int64_t slot = a.slot_bytes;
  const int64_t bs = a.block;
  const bool rel = a.fence & 1, acq = a.fence & 2;
  const int Pm1 = P - 1;
  const int nu = Pm1 * a.nch;

  entry_guard(a, ctl, r, epoch, kHazS | kHazR, -1, deadline, err);
  if (r == root) {
    const char* const in = a.in[y];
    // units [0, nu): block j into j's S slot [root]; [nu, 2 nu): the own block into j's R slot
    // [root]. The scattered blocks go first: their owners forward them.
    for (int u = blockIdx.x; u < 2 * nu; u += G) {
      const bool own = u >= nu;
      const int v = own ? u - nu : u;
      const int c = v / Pm1;
      const int j = (root + 1 + v % Pm1) % P;
      const int b = own ? root : j;
      const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
      const int64_t len = chunk_len(a, b, c);
      char* dst = a.base[j] + (own ? a.off_R : a.off_S) + root * slot + cstart * es;
      if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err))
        copy_to_slab<E>(dst, in + (static_cast<int64_t>(b) * bs + cstart) * es, len);
      publish_flags([&](int) { return own ? f2(a, j, root, c) : f1(a, j, root, c); }, 1, epoch, rel);
    }
    // every peer has entered this launch (and so finished the one before)
    if (blockIdx.x == 0)
      wait_flags([&](int s) -> const uint32_t* { return s == root ? nullptr : f2(a, root, s, 0); }, P, epoch, deadline,
                 err, ERR_TIMEOUT_BARRIER, false);
  } else {
    char* const out = a.out[y];
    if (blockIdx.x == 0 && threadIdx.x == 0) st_flag(f2(a, root, r, 0), epoch);
    read_delay(a, r);
    // own block: out of the S slot [root] into `out` (k == r) and on into the R slot [r] of
    // every other non-root k
    for (int u = blockIdx.x; u < P * a.nch; u += G) {
      const int c = u / P;
      const int k = (r + u % P) % P;
      if (k == root) continue;
      const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
      const int64_t len = chunk_len(a, r, c);
      wait_flags([&](int) -> const uint32_t* { return f1(a, r, root, c); }, 1, epoch, deadline, err,
                 ERR_TIMEOUT_SCATTER, acq);
      const char* src = a.base[r] + a.off_S + root * slot + cstart * es;
      char* dst = k == r ? out + (static_cast<int64_t>(r) * bs + cstart) * es
                         : a.base[k] + a.off_R + r * slot + cstart * es;
      if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err)) copy_from_slab<E>(dst, src, len);
      if (k != r) publish_flags([&](int) { return f2(a, k, r, c); }, 1, epoch, rel);
    }
    // block of source s (the root's own block, the others' forwards) out of the R slot [s]
    for (int u = blockIdx.x; u < nu; u += G) {
      const int c = u / Pm1;
      const int s = (r + 1 + u % Pm1) % P;
      const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
      const int64_t len = chunk_len(a, s, c);
      wait_flags([&](int) -> const uint32_t* { return f2(a, r, s, c); }, 1, epoch, deadline, err,
                 ERR_TIMEOUT_SCATTER, acq);
      if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err))
        copy_from_slab<E>(out + (static_cast<int64_t>(s) * bs + cstart) * es,
                          a.base[r] + a.off_R + s * slot + cstart * es, len);
    }
  }
  finish_launch_done(a, ctl, epoch, r, kHazS | kHazR);
}

// in[y] on every rank; out[y] is written on the root only.
template <class E, int PT>
__global__ __launch_bounds__(kCommThreads) void reduce_kernel(CommArgs a) {
  constexpr int es = 16 / E::ELEMS;
  const int P = a.P;
  const int y = blockIdx.y;
  const int r = a.rank0 + y;
  const int root = a.root;
  const char* const in = a.in[y];
  uint32_t* const ctl = a.ctl[y];
  uint32_t* const err = &ctl[2];
  const uint32_t epoch = launch_epoch(ctl);
  const uint64_t deadline = wall_ticks() + a.timeout;
  const int G = gridDim.x;
  const int64_t slot = a.slot_bytes;
  const int64_t bs = a.block;
  const bool rel = a.fence & 1, acq = a.fence & 2;
  const int Pm1 = P - 1;
  const int nu = Pm1 * a.nch;
  const int nu2 = a.nch * a.sub;

  // Phase 1 (the reduce-scatter's): block j of the input into j's S slot [r]. The R slots are
  // written after this rank heard from the root in this launch: no guard for them.
  if (static_cast<int>(blockIdx.x) < nu) entry_guard(a, ctl, r, epoch, kHazS, -1, deadline, err);
  for (int u = blockIdx.x; u < nu; u += G) {
    const int c = u / Pm1;
    const int j = (r + 1 + u % Pm1) % P;
    const int64_t cstart = static_cast<int64_t>(c) * a.chunk;
    const int64_t len = chunk_len(a, j, c);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, c, err))
      copy_to_slab<E>(a.base[j] + a.off_S + r * slot + cstart * es,
                      in + (static_cast<int64_t>(j) * bs + cstart) * es, len);
    publish_flags([&](int) { return f1(a, j, r, c); }, 1, epoch, rel);
  }

  read_delay(a, r);
  // Phase 2: own block = own input + the P-1 received contributions, each chunk in `sub`
  // pieces; the root reduces into `out`, rank j into the root's R slot [j] (flag per piece)
  for (int u = blockIdx.x; u < nu2; u += G) {
    const int c = u / a.sub;
    const int q = u % a.sub;
    const int64_t cstart = static_cast<int64_t>(c) * a.chunk + static_cast<int64_t>(q) * a.subchunk;
    const int64_t len = clamp_len(chunk_len(a, r, c) - static_cast<int64_t>(q) * a.subchunk, a.subchunk);
    wait_flags([&](int s) -> const uint32_t* { return s == r ? nullptr : f1(a, r, s, c); }, P, epoch, deadline, err,
               ERR_TIMEOUT_SCATTER, acq);
    if (len > 0 && unit_in_bounds(a, cstart * es, len * es, u, err)) {
      const RedSrc src{in + (static_cast<int64_t>(r) * bs + cstart) * es, a.base[r] + a.off_S + cstart * es, slot, r};
      char* o = r == root ? a.out[y] + (static_cast<int64_t>(r) * bs + cstart) * es
                          : a.base[root] + a.off_R + r * slot + cstart * es;
      reduce_to<E, PT>(P, src, 1, r == root ? 0 : -1, [&](int) -> char* { return o; }, len, a.scale, a.fence & 1);
    }
    if (r != root) publish_flags([&](int) { return f2(a, root, r, u); }, 1, epoch, rel);
  }
  // Phase 3 (root): the reduced block of source s out of the R slot [s]
  if (r == root) {
    char* const out = a.out[y];
    for (int w = blockIdx.x; w < Pm1 * nu2; w += G) {
      const int u = w / Pm1;
      const int s = (r + 1 + w % Pm1) % P;
      const int c = u / a.sub;
      const int q = u % a.sub;
      const int64_t cstart = static_cast<int64_t>(c) * a.chunk + static_cast<int64_t>(q) * a.subchunk;
      const int64_t len = clamp_len(chunk_len(a, s, c) - static_cast<int64_t>(q) * a.subchunk, a.subchunk);
      wait_flags([&](int) -> const uint32_t* { return f2(a, r, s, u); }, 1, epoch, deadline, err, ERR_TIMEOUT_REDUCE,
                 acq);
      if (len > 0 && unit_in_bounds(a, cstart * es, len * es, u, err))
        copy_from_slab<E>(out + (static_cast<int64_t>(s) * bs + cstart) * es,
                          a.base[r] + a.off_R + s * slot + cstart * es, len);
    }
  }
  finish_launch_done(a, ctl, epoch, r, kHazS | kHazR);
}

void launch_rooted(const CommArgs& a, dim3 grid, hipStream_t s, DType dt, Rooted kind) {
  dispatch_dtype(static_cast<int>(dt), [&](auto tag) {
    using E = decltype(tag);
    if (kind == Rooted::Broadcast) {
      hipLaunchKernelGGL((broadcast_kernel<E>), grid, dim3(kCommThreads), 0, s, a);
    } else {
      switch (a.P) {
        case 2: hipLaunchKernelGGL((reduce_kernel<E, 2>), grid, dim3(kCommThreads), 0, s, a); break;
        case 4: hipLaunchKernelGGL((reduce_kernel<E, 4>), grid, dim3(kCommThreads), 0, s, a); break;
        case 8: hipLaunchKernelGGL((reduce_kernel<E, 8>), grid, dim3(kCommThreads), 0, s, a); break;
        default: hipLaunchKernelGGL((reduce_kernel<E, 0>), grid, dim3(kCommThreads), 0, s, a); break;
      }
    }
  });
}

}  // namespace mxar
