// constrain_plan_main.cpp -- the host-only logic of the constraint pass
// (raft-tla_amd/csrc/rtla_constrain.h: the chunk size from the environment's
// text, the chunk plan, the batch ring's argument check) as a stand-alone host
// program, for a sanitizer build (tests/test_constrain_host.py).  The plan is
// walked as rtla_constrain.cpp walks it, over buffers of exactly the sizes it
// allocates: an index past one of them is a read or write past an allocation.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtla_constrain.h"

using namespace rtla;

#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                              \
    }                                                        \
  } while (0)

static int plan(uint64_t n, uint64_t R, uint64_t level_rows) {
  std::vector<uint64_t> keep(((level_rows > 1 ? level_rows : 1) + 63) / 64, 0);  // constrain_alloc's keep bitmap
  std::vector<uint32_t> offs(R / 64, 0), masks(R, 0);
  uint64_t next = 0;
  for (uint64_t c = 0; c < constrain_chunks(n, R); c++) {
    const ConstrainChunk ch = constrain_chunk(n, R, c);
    CHECK(ch.first == next && ch.first % 64 == 0 && ch.rows >= 1 && ch.rows <= R);
    CHECK(c + 1 == constrain_chunks(n, R) || ch.rows == R);
    for (uint64_t i = 0; i < ch.rows; i++) masks[i] = 1;                  // launch_pred's masks
    uint64_t* const words = keep.data() + ch.first / 64;                 // launch_constrain_pack's keep words
    for (uint64_t g = 0; g < (ch.rows + 63) / 64; g++) {
      words[g] = ~0ull;
      offs[g] = (uint32_t)(g * 64);                                      // k_constrain_scan's offsets
    }
    next += ch.rows;
  }
  CHECK(next == n);
  CHECK(constrain_chunk(n, R, constrain_chunks(n, R)).rows == 0);
  return 0;
}

int main() {
  // the chunk size from text: whole groups of 64 within [64, max]; anything that is no number: the default
  struct { const char* text; uint64_t rows; } texts[] = {
      {nullptr, CONSTRAIN_CHUNK_DEFAULT}, {"", CONSTRAIN_CHUNK_DEFAULT}, {"0", CONSTRAIN_CHUNK_DEFAULT},
      {"x", CONSTRAIN_CHUNK_DEFAULT}, {"12x", CONSTRAIN_CHUNK_DEFAULT}, {" ", CONSTRAIN_CHUNK_DEFAULT},
      {"-5", CONSTRAIN_CHUNK_DEFAULT}, {"1", 64}, {"63", 64}, {"64", 64}, {"65", 128}, {"128", 128}, {"4096", 4096},
      {"1000000", 1000000}, {"1000001", 1000064}, {"16777216", CONSTRAIN_CHUNK_MAX}, {"16777217", CONSTRAIN_CHUNK_MAX},
      {"18446744073709551615", CONSTRAIN_CHUNK_MAX}, {"99999999999999999999999999", CONSTRAIN_CHUNK_MAX}};
  for (auto& t : texts) {
    std::string copy = t.text ? t.text : "";  // (an exact-size copy: a read past the text's end is caught)
    const uint64_t got = constrain_chunk_rows(t.text ? copy.c_str() : nullptr);
    if (got != t.rows) fprintf(stderr, "chunk rows of \"%s\": %llu\n", copy.c_str(), (unsigned long long)got);
    CHECK(got == t.rows && got % 64 == 0 && got >= 64 && got <= CONSTRAIN_CHUNK_MAX);
  }
  for (uint64_t v : {0ull, 1ull, 63ull, 64ull, 65ull, 1ull << 20, (1ull << 24) - 1, 1ull << 24, ~0ull}) {
    const uint64_t got = constrain_chunk_rows(v);
    CHECK(got % 64 == 0 && got >= 64 && got <= CONSTRAIN_CHUNK_MAX && (v == 0 || got >= v || got == CONSTRAIN_CHUNK_MAX));
  }
  // the plan: the chunks tile [0, n) in order, every index inside the buffers made for it
  const uint64_t sizes[] = {1, 63, 64, 65, 127, 128, 129, 1000, 4096, 4097, 70000};
  for (uint64_t n : sizes)
    for (uint64_t R : {64ull, 128ull, 4096ull, 1ull << 16})
      for (uint64_t slack : {0ull, 64ull})
        if (plan(n, R, ((n + 63) & ~63ull) + slack)) return 1;
  CHECK(constrain_chunks(0, 64) == 0);
  // the batch ring
  CHECK(constrain_ring_ok(0, 64, 0) && constrain_ring_ok(64, 64, 0) && constrain_ring_ok(1000, 1088, 1024));
  CHECK(!constrain_ring_ok(65, 64, 0) && !constrain_ring_ok(1, 0, 0) && !constrain_ring_ok(1, 100, 0));
  CHECK(!constrain_ring_ok(1, 128, 32) && !constrain_ring_ok(1, 128, 128) && !constrain_ring_ok(1, 1ull << 40, 0));
  CHECK(!constrain_ring_ok(~0ull, 1ull << 32, 0) && !constrain_ring_ok(~0ull - 10, 64, 0));
  printf("constrain plan: ok\n");
  return 0;
}
