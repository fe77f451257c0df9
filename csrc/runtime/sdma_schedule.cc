#include "sdma_schedule.h"

#include <algorithm>
#include <stdexcept>
#include <utility>

#include "launch_geometry.h"

namespace mxar {

namespace {
int64_t rup(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace

int64_t sdma_slot_bytes(int64_t requested) { return rup(std::max<int64_t>(requested, 4096), 4096); }

int64_t sdma_slab_bytes(int world, int64_t slot_bytes) {
  return ipc_safe_bytes(kFlagBytes + 4 * static_cast<int64_t>(world) * slot_bytes);
}

int64_t sdma_segment_elems(int world, int64_t slot_bytes, int64_t es) { return world * (slot_bytes / es); }

SdmaSegment plan_sdma_segment(int world, int64_t n, int64_t es, int64_t slot_bytes, int pieces) {
  const int64_t elems = 16 / es;
  SdmaSegment s;
  s.n = n;
  s.block = rup(cdiv(n, world), elems);
  if (s.block * es > slot_bytes) throw std::logic_error("SdmaComm: segment exceeds the slot");
  const int want = pieces > 0 ? std::min(pieces, kSdmaMaxPieces)
                              : static_cast<int>(std::clamp<int64_t>(cdiv(s.block * es, kPieceBytes), 2, kSdmaMaxPieces));
  s.pe = rup(cdiv(s.block, want), std::max<int64_t>(elems, 4096 / es));
  s.K = static_cast<int>(std::max<int64_t>(1, cdiv(s.block, s.pe)));
  return s;
}

SdmaParts sdma_parts(int64_t bytes, int epp) {
  SdmaParts p;
  if (bytes <= 0) return p;
  p.bytes = bytes;
  p.size = rup(cdiv(bytes, std::max(1, epp)), 4096);
  p.count = static_cast<int>(cdiv(bytes, p.size));
  return p;
}

std::vector<uint32_t> sdma_engine_ids(uint32_t mask) {
  std::vector<uint32_t> ids;
  for (int b = 0; b < 32; ++b)
    if (mask & (1u << b)) ids.push_back(1u << b);
  return ids;
}

uint32_t sdma_engine_share(uint32_t local_engines, int nloc, int rank) {
  const std::vector<uint32_t> ids = sdma_engine_ids(local_engines);
  uint32_t mine = 0;
  for (size_t i = 0; i < ids.size(); ++i)
    if (static_cast<int>(i % nloc) == rank) mine |= ids[i];
  return mine;
}

int sdma_auto_epp(int n_engines, int world) { return std::max(1, n_engines / std::max(1, world - 1)); }

std::vector<uint32_t> sdma_pick_engines(uint32_t avail_mask, uint32_t allowed, int k, int epp) {
  // a direction the query knows nothing of: the local engines
  const std::vector<uint32_t> avail = sdma_engine_ids((avail_mask & allowed) != 0 ? avail_mask & allowed : allowed);
  std::vector<uint32_t> out;
  for (int p = 0; p < epp && !avail.empty(); ++p) out.push_back(avail[(static_cast<size_t>(k) * epp + p) % avail.size()]);
  return out;
}

SdmaSchedule plan_sdma_copies(const SdmaSegment& seg, int world, int rank, int64_t es, int epp, int64_t slot_bytes,
                              int par, SdmaSchedule scratch) {
  SdmaSchedule s = std::move(scratch);
  const int W = world, r = rank, K = seg.K;
  s.copies.clear();
  auto flag = [&](int dst, int64_t word, SdmaSigRef dep, SdmaSig done, int peer, int engine) {
    s.copies.push_back({dst, 4 * word, SdmaSrc::Epoch, 0, 4, dep, {done, 0}, peer, engine});
  };
  // the parts of piece k of block j: to `dst`'s slot at `slot_off`, from `src` (block j of it)
  auto parts = [&](int j, int k, int dst, int64_t slot_off, SdmaSrc src, SdmaSigRef dep, SdmaSigRef done) {
    const SdmaParts ps = sdma_parts(seg.piece_len(j, k) * es, epp);
    const int64_t at = static_cast<int64_t>(k) * seg.pe * es;
    for (int p = 0; p < ps.count; ++p)
      s.copies.push_back({dst, slot_off + at + ps.off(p), src, static_cast<int64_t>(j) * seg.block * es + at + ps.off(p),
                          ps.len(p), dep, done, dst, p});
    return ps.count;
  };
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < W; ++j) {
      if (j == r || k >= seg.pieces_of(j)) continue;
      const SdmaSigRef done{SdmaSig::C1, j * K + k};
      const int n = parts(j, k, j, sdma_sd_off(W, slot_bytes, par, r), SdmaSrc::In, {SdmaSig::Start, 0}, done);
      flag(j, sdma_fs_word(r, k), done, SdmaSig::Scf, j, std::max(0, n - 1));
    }
  for (int k = 0; k < seg.pieces_of(r); ++k) {
    const SdmaSigRef done{SdmaSig::C2, k};
    for (int q = 0; q < W; ++q)
      if (q != r) parts(r, k, q, sdma_rd_off(W, slot_bytes, par, r), SdmaSrc::Out, {SdmaSig::Mid, k}, done);
    for (int q = 0; q < W; ++q)
      if (q != r) flag(q, sdma_fr_word(r, k), done, SdmaSig::Gdf, q, 0);
    // the own FR[r][k] once every phase-2 part of the piece has completed: the engines read
    // the own block of the output for them, so the call may not count as done (and the caller
    // may not write the output) before they are - the gather kernel waits for this word with
    // the peers'
    if (W < 2) break;
    flag(r, sdma_fr_word(r, k), done, SdmaSig::Gdf, (r + 1) % W, 0);
  }
  s.c1.assign(static_cast<size_t>(W) * K, 0);
  s.c2.assign(static_cast<size_t>(K), 0);
  s.scf = s.gdf = 0;
  for (const SdmaCopy& c : s.copies) switch (c.done.kind) {
      case SdmaSig::C1: ++s.c1[static_cast<size_t>(c.done.index)]; break;
      case SdmaSig::C2: ++s.c2[static_cast<size_t>(c.done.index)]; break;
      case SdmaSig::Scf: ++s.scf; break;
      case SdmaSig::Gdf: ++s.gdf; break;
      default: break;
    }
  return s;
}

}  // namespace mxar
