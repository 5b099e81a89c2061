// rtla_constrain.h -- what the constraint pass's host unit (rtla_constrain.cpp)
// and its kernels (rtla_kconstrain.hip) share: the running totals the kernels
// keep on the device, and the host-only chunk planning and argument checks
// (plain C++: tests/constrain_plan_main.cpp builds them under a sanitizer).
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace rtla {

// Rows of one compaction chunk: RTLA_CONSTRAIN_CHUNK's, or this.  A chunk is whole 64-row groups.
constexpr uint64_t CONSTRAIN_CHUNK_DEFAULT = 1ull << 20;
constexpr uint64_t CONSTRAIN_CHUNK_MAX = 1ull << 24;  // (the staging buffer: 2^24 rows of 43 words are 2.9 GB)

// The device's running totals of one rtla_pred_constrain call.  Written by the single block of k_constrain_scan,
// read by the gather and copy-back kernels that follow it in the stream; dropped is the keep-bitmap pass's tally.
struct ConstrainTotals {
  unsigned long long base;     // kept rows of the chunks before the current one: where its kept rows go
  unsigned long long kept;     // kept rows of the current chunk
  unsigned long long dropped;  // rows of the level on which some definition is false
  unsigned long long move;     // 0: the current chunk keeps every row where it lies (nothing is copied)
};

// `text` (RTLA_CONSTRAIN_CHUNK, may be null) as a chunk size: rows, rounded up to whole groups of 64 and held
// within [64, CONSTRAIN_CHUNK_MAX]; null, empty, zero or no number: the default.
inline uint64_t constrain_chunk_rows(const char* text) {
  if (!text || !*text || *text == '-') return CONSTRAIN_CHUNK_DEFAULT;
  char* end = nullptr;
  const unsigned long long v = strtoull(text, &end, 10);
  if (end == text || *end || v == 0) return CONSTRAIN_CHUNK_DEFAULT;
  if (v >= CONSTRAIN_CHUNK_MAX) return CONSTRAIN_CHUNK_MAX;
  return (v + 63) & ~63ull;
}
// The same for a chunk size given as a number (rtla_constrain_batch): 0 = the default.
inline uint64_t constrain_chunk_rows(uint64_t v) {
  if (v == 0) return CONSTRAIN_CHUNK_DEFAULT;
  if (v >= CONSTRAIN_CHUNK_MAX) return CONSTRAIN_CHUNK_MAX;
  return (v + 63) & ~63ull;
}

// Chunk c of a level of n rows cut into chunks of R rows: its first row and its rows (the last may be short).
struct ConstrainChunk {
  uint64_t first, rows;
};
inline uint64_t constrain_chunks(uint64_t n, uint64_t R) { return (n + R - 1) / R; }
inline ConstrainChunk constrain_chunk(uint64_t n, uint64_t R, uint64_t c) {
  const uint64_t first = c * R;
  return ConstrainChunk{first, first < n ? (n - first < R ? n - first : R) : 0};
}

// rtla_constrain_batch's ring: whole 64-row groups, room for the rows' groups, a start inside it on a group
// boundary -- what Ring asks of the arena (a group of 64 rows never wraps).
inline bool constrain_ring_ok(uint64_t n, uint64_t ring_cap, uint64_t ring_start) {
  if (n > ring_cap) return false;
  const uint64_t need = (n + 63) & ~63ull;
  return ring_cap >= 64 && ring_cap % 64 == 0 && ring_cap >= need && ring_cap <= (1ull << 32) &&
         ring_start % 64 == 0 && ring_start < ring_cap;
}

}  // namespace rtla
