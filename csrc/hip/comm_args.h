// What the host hands to the data-plane kernels: the launch arguments of every fused kernel
// (CommArgs), the door entries and group members of the resident threshold kernels. Plain
// structs - this header is included by host code built without the HIP compiler
// (xgmi_comm.cc, xgmi_plane.cc) and by the kernels (xgmi_device.h). CommArgs is the
// kernel-argument ABI: field order and types are fixed (the static_asserts below).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../runtime/launch_geometry.h"

namespace mxar {

// Resident rounds (xgmi_threshold.hip threshold_resident_kernel; xgmi_plane.cc): the host
// posts each round as one 64-B entry of a door ring in pinned host memory, the sequence word
// written last; a kernel that stays on the GPU between rounds runs them.
struct ResidentDoor {
  uint64_t in, out, counts, counts_host, err_out, done_out;  // device-visible addresses
  uint32_t epoch;
  int32_t cmd;  // kResRound / kResCold / kResStop
  uint32_t seq;
  uint32_t check;  // door_check(entry): the kernel reads the whole entry in one 64-B load and
                   // takes it only when the check matches (no second read after the sequence word)
};
constexpr int kResidentDoors = 64;
// A mix of the entry's words and its sequence number (host and device compute the same).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t door_check(const uint32_t* w14, uint32_t seq) {
  uint32_t h = seq * 0x9E3779B1u + 0x7F4A7C15u;
  for (int i = 0; i < 14; ++i) {
    h = (h ^ w14[i]) * 0x85EBCA6Bu;
    h ^= h >> 13;
  }
  return h ^ (h >> 16);
}
enum : int32_t { kResRound = 0, kResCold = 1, kResStop = 2 };
// host state words the kernel writes: [0] kResRunning / kResExiting / kResExited, [1] the
// last entry it consumed (its door slot may be reused)
enum : uint32_t { kResRunning = 0, kResExiting = 1, kResExited = 2 };

// Group resident rounds (xgmi_threshold.hip threshold_group_resident_kernel; xgmi_plane.cc
// PlaneGroup): the co-located workers of one job share ONE resident kernel, a slice of
// workgroups per worker, each fed from that worker's own door ring by a dispatcher wave.
struct GroupResidentMember {
  const ResidentDoor* door;  // the worker's pinned door ring (device-visible address)
  uint32_t* hstate;          // its pinned words: [1] the last entry consumed
  uint64_t* dm;              // its device words: [0] go, [2..9] the entry handed to its slice
  const uint32_t* hforce;    // its pinned force / abort words
  const uint32_t* habort;
  uint64_t* stamps;          // its phase-stamp buffer (study knob; null = off)
  uint64_t* split_dec;       // its split-chunk scratch (RoundSpec::split_scratch; null = unsplit)
  uint32_t* split_ctr;
  uint32_t* split_early;
  uint32_t seq0;             // the first entry this launch takes
  int rank;
};

// One launch serves one rank (one process per GPU: gridDim.y == 1, rank = rank0) or all
// P logical ranks of a single-process cluster on one device (gridDim.y == P, rank =
// rank0 + blockIdx.y): every rank's workgroups are then co-resident in ONE dispatch, so
// no rank can be starved behind another on a shared hardware queue.
struct CommArgs {
  const char* in[kMaxRanks];
  char* out[kMaxRanks];
  // per rank: [0] epoch [1] ticket [2] error; threshold rounds: [3] completion / late-ticket
  // counter [4] round count [5] early arrivals [6] snapshot barrier [7] early tickets
  uint32_t* ctl[kMaxRanks];
  int64_t n;      // elements in this segment
  int64_t block;  // elements per block (two-shot) / whole segment (one-shot)
  int64_t chunk;  // elements per chunk (scatter / gather work unit)
  int64_t subchunk;  // elements per reduce work unit (chunk split `sub` ways)
  int nch;        // chunks per block
  int sub;        // reduce units per chunk
  int P;
  int rank0;
  int fence;      // bit0: system release before flags, bit1: system acquire after waits
  float scale;    // applied to the fp32 sum before rounding (1 = sum, 1/P = mean)
  int64_t maxch;
  int64_t off_S, off_R, slot_bytes;  // slot_bytes: the slot STRIDE in the slab (capacity + pad)
  int64_t slot_cap;                   // usable bytes per slot
  uint64_t timeout;
  char* base[kMaxRanks];
  // threshold kernel (xgmi_threshold.hip); rows = 1 for the other kernels
  int rows;            // S/R slot rows in the slab: row 0 (lock-step kernels) + trows
  int trows;           // threshold lag ring: rows 1..trows (maxLag + 1; 0 = not allocated)
  int full;            // thReduce = thComplete = 1: every contribution and chunk is taken
  int min_reduce;      // contributions per chunk that complete a reduce (thReduce)
  int64_t min_complete;  // reduced chunks that complete the round (thComplete)
  int32_t* counts;     // optional [P][nch] contributions per output chunk (0 = missing)
  int rescale;         // scale a chunk reduced from cnt contributions by P / cnt
  // protocol-engine rounds (xgmi_plane.cc, RoundSpec): explicit round epoch (0 = ctl[4] + 1),
  // forced-cold round (no own contribution, nothing waited for), the reference's
  // arrival-order accounting, and the pinned host word the engine raises on a catch-up
  uint32_t epoch_set;
  int cold;
  int order_ref;
  const uint32_t* hforce;
  const uint32_t* habort;  // pinned host word: rounds <= this epoch are abandoned (threshold kernel)
  uint32_t* err_out;  // optional: the round's error word, written by the last workgroup (pinned host)
  uint32_t* done_out;  // optional: set to the epoch by the last workgroup after its release (pinned host)
  // optional: where the last workgroup copies `counts` (P x nch int32, pinned host) once the
  // round is done - every workgroup writes its counts to device memory (`counts`), so no
  // unit waits on a PCIe write acknowledgement
  int32_t* counts_host;
  // low-latency one-shot (xgmi_ll.hip): slots [parity][src] of ll_slot bytes at off_LL
  int64_t off_LL, ll_slot;
  // fused reduce-scatter + AdamW + all-gather (xgmi_adam.hip): per rank fp32 shard state
  float* opt_p[kMaxRanks];
  float* opt_m[kMaxRanks];
  float* opt_v[kMaxRanks];
  float lr, beta1, beta2, eps, wd, c1, c2_sqrt;  // c1 = 1 - beta1^t, c2_sqrt = sqrt(1 - beta2^t)
  // phase profile (MXAR study knob, XgmiComm::set_phase_stamps): per (rank y, workgroup x)
  // kPhaseSlots s_memrealtime values - see PhaseStamps (xgmi_device.h)
  uint64_t* stamps;
  uint64_t delay;      // test knob: ticks rank `delay_rank` idles before phase 1
  int delay_rank;
  // test knob (XgmiComm::set_read_delay): ticks rank `rdelay_rank` idles before the phase that
  // reads what peers pushed - holds a slow reader inside its launch (slot-reuse tests)
  uint64_t rdelay;
  int rdelay_rank;
  // test knob (XgmiComm::set_forward_delay): ticks rank `fdelay_rank` idles before the ring's
  // LAST all-gather forward (its late flag then races the next kernel's flags - the flag
  // ownership test, tests/test_comm_gpu.py)
  uint64_t fdelay;
  int fdelay_rank;
  int noguard;  // MXAR_SLOT_GUARD=0: skip entry_guard (A/B of its cost and negative control only)
  int ring_hop_rows;  // study only (MXAR_RING_FLAGS=hop): the pre-fix ring flag layout, row = hop index
  // threshold kernel with sub > 1 (chunks split into `sub` slices of `subchunk` elements,
  // one workgroup each): the rank's own scratch, zeroed when the membership is configured.
  // split_dec: 64-bit decision words, [c] own reduce chunk c, [maxch + j * maxch + c] gather
  // unit (j, c); split_ctr: slice counters, [c] reduce, [maxch + j * maxch + c] scatter;
  // split_early: [j * maxch + c] = epoch when gather unit (j, c) was in at launch
  int sgroup;  // threshold kernel, unsplit chunks: chunks per scatter unit (one copy, one release)
  // threshold kernel: the lag gate of round e may be taken as open when this rank's round e - 1
  // was clean (it gathered every peer's reduced chunk of e - 1, so every peer had finished
  // e - 2). Set by the host when that proof holds: trows >= 2 and every rank's block holds at
  // least one chunk or the thresholds are full (plan_threshold, launch_geometry.cc).
  int gate_shortcut;
  // threshold kernel, protocol rounds with thresholds that tolerate a missing peer (unsplit
  // chunks only): a peer still inside the round that last used this round's row after
  // `lag_wait` ticks at the lag gate is SKIPPED for the round - nothing is written into its
  // slab (its FORCE request still is), so a straggler never holds the fast ranks back. The
  // laggard's late writes land in its own slots of our slab under older epochs, which no
  // round of ours takes (xgmi_threshold.hip, lag gate). 0 = wait (the bounded-buffer gate).
  int lag_skip;
  uint64_t lag_wait;
  // threshold kernel, full thresholds: the one-shot body (xgmi_threshold.hip) - every rank
  // pushes its whole input as low-latency units and reduces every chunk itself (small rounds)
  int oneshot;
  // rooted collectives (xgmi_rooted.hip): the rank that holds the tensor (broadcast) or
  // receives the sum (reduce); 0 for every other kernel
  int root;
  uint64_t* split_dec;
  uint32_t* split_ctr;
  uint32_t* split_early;
  // clipped step (xgmi_clip.hip), per rank. Both halves: the fp32 gradient shard (block_elems
  // elements, block `rank`). Reduce-scatter half: one partial sum of squares per reduce unit
  // (nch * sub floats of scratch) and where the rank's sum of squares goes. Update half: the
  // clip coefficient (one fp32, read by every workgroup).
  float* gshard[kMaxRanks];
  float* sq_part[kMaxRanks];
  float* sq_out[kMaxRanks];
  const float* coef[kMaxRanks];
};

// Loss-scaled step (xgmi_scale.hip). The step record: what the one-wave step-control kernel
// decides between the two halves of the split step and the record-driven update half
// (xgmi_clip.hip) reads instead of CommArgs::coef / c1 / c2_sqrt. 32 bytes, 16-byte aligned, one
// per rank, in ordinary device memory; `coef` comes first, so CommArgs::coef[y] points at it.
struct StepRecord {
  float coef;      // clip / scale: what the update half multiplies the fp32 shard by
  uint32_t skip;   // 1: a non-finite sum of squares - the update half writes nothing
  float c1;        // AdamW's bias corrections at the applied count, from the host's table
  float c2_sqrt;
  float norm;      // the norm of the unscaled gradient
  float clip;      // min(1, max_norm / (norm + 1e-6)), 1.0f when not clipping
  uint32_t short_table;  // 1: the applied count passed the filled part of the table (a host bug)
  uint32_t pad;
};
static_assert(sizeof(StepRecord) == 32 && offsetof(StepRecord, coef) == 0, "the step record is read by offset");
// The scaler's device state, updated in place by the control kernel: four 32-bit words.
struct ScaleState {
  float scale;
  int32_t tracker;  // clean steps since the scale last changed
  int32_t applied;  // steps that updated the parameters: AdamW's t
  int32_t skipped;
};
static_assert(sizeof(ScaleState) == 16, "the scaler state is viewed as four words");
struct ScaleStepArgs {
  const double* recs;  // [P][2]: the ranks' 16-byte records in rank order, [k][0] = sum of squares
  int P;
  int clip;            // 0: clip = 1.0f
  float max_norm;
  int dynamic;         // 0: a static scale
  float growth, backoff;
  int interval;
  ScaleState* state;
  StepRecord* rec;
  const float* table;  // (c1, c2_sqrt) of count t at [2 (t - 1)], t = 1 .. filled
  int end;             // the count from which both corrections are 1.0f: the index clamps there
  int filled;          // counts the host has filled so far (<= end)
};

// A plane group's resident kernel (threshold_group_resident_kernel): y = 0 is the dispatcher
// row, y = 1 + k worker k's slice.
struct GroupResArgs {
  GroupResidentMember m[kMaxRanks];
  uint32_t* gstate;  // pinned: [0] kResRunning / kResExiting / kResExited (the group's kernel)
  uint64_t* gdm;     // device: [0] the dispatcher's heartbeat (100 MHz ticks)
  uint64_t idle;     // ticks without a round before the kernel leaves
  uint32_t gen;      // launch generation (the go words of a relaunched kernel differ)
  int Y;             // workers
};
static_assert(sizeof(CommArgs) + sizeof(GroupResArgs) <= 4096, "threshold_group_resident_kernel arguments exceed 4 KiB");
// the kernels read these by offset: a reorder or a changed type must fail the build
static_assert(sizeof(CommArgs) == 1760, "CommArgs is the kernel-argument ABI");
static_assert(offsetof(CommArgs, stamps) == 1136 && offsetof(CommArgs, oneshot) == 1216 &&
                  offsetof(CommArgs, split_early) == 1240 && offsetof(CommArgs, gshard) == 1248,
              "CommArgs is the kernel-argument ABI");

}  // namespace mxar
