// rtla_ckpt.cpp -- checkpoint / recover (TLC's -checkpoint / -recover and its
// states/ directory, reference .gitignore:2).  One file per shard:
// <prefix>.shard<id>.rtla = header | fingerprint set | sent cache (G > 1) |
// parent records [0, cur_base + n_cur) | current frontier rows | coverage.
// Written between levels; a context opened with the same configuration
// (same cfg, fingerprint-set size and shard count) resumes from it.
#include <unistd.h>

#include <string>

#include "rtla_ctx.h"

namespace {
struct CkptHeader {
  char magic[8];
  int32_t abi, nshard, shard, W, tlog2, level;
  rtla_cfg cfg;
  uint64_t distinct, generated, max_front, cur_base, n_cur, parents_n;
  int32_t finished, viol_mask, viol_in_model, viol_inst;
  uint64_t viol_parent, viol_child;
};

bool write_all(FILE* f, const void* p, size_t n) { return fwrite(p, 1, n, f) == n; }
bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

// device <-> file through a bounded host staging buffer
bool dev_to_file(FILE* f, const void* d, size_t n, std::vector<char>& buf) {
  for (size_t off = 0; off < n; off += buf.size()) {
    const size_t m = std::min(buf.size(), n - off);
    if (hipMemcpy(buf.data(), (const char*)d + off, m, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (!write_all(f, buf.data(), m)) return false;
  }
  return true;
}
bool file_to_dev(FILE* f, void* d, size_t n, std::vector<char>& buf) {
  for (size_t off = 0; off < n; off += buf.size()) {
    const size_t m = std::min(buf.size(), n - off);
    if (!read_all(f, buf.data(), m)) return false;
    if (hipMemcpy((char*)d + off, buf.data(), m, hipMemcpyHostToDevice) != hipSuccess) return false;
  }
  return true;
}
bool ring_to_file(FILE* f, const Ring& r, int W, uint64_t n, std::vector<char>& buf) {
  for (uint64_t g = 0; g < n;) {
    const uint64_t p = ring_idx(r, g), m = std::min<uint64_t>(n - g, r.cap - p);
    if (!dev_to_file(f, r.base + p * (uint64_t)W, m * W * 4, buf)) return false;
    g += m;
  }
  return true;
}
std::string ckpt_path(const char* prefix, int shard) {
  return std::string(prefix) + ".shard" + std::to_string(shard) + ".rtla";
}
}  // namespace

// Collective when world > 1: every rank reaches every reduction below, also
// after a local failure (its flag travels in the reduction), so one rank's
// error is every rank's error and no rank is left waiting in a collective.
extern "C" int rtla_checkpoint(rtla_ctx* x, const char* prefix) {
  if (!x || !prefix) return RTLA_E_ARG;
  if (!x->inited || x->seeded) return RTLA_E_STATE;  // (the files hold no roots: a seeded search stays in memory)
  std::vector<char> buf(64 << 20);
  // Each shard is written to <path>.tmp (flushed to disk); only when every
  // shard of every rank has been written are the files renamed over the
  // previous checkpoint, so a crash mid-write leaves the last good one intact.
  uint64_t failed = hipSetDevice(x->device) != hipSuccess || hipStreamSynchronize(x->stream) != hipSuccess ? 1 : 0;
  for (auto& s : x->sh) {
    if (failed) break;
    CkptHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "RTLACKP1", 8);
    h.abi = RTLA_ABI_VERSION; h.nshard = x->nshard; h.shard = s.id; h.W = x->L.W; h.tlog2 = x->tlog2;
    h.level = x->level; h.cfg = x->cfg;
    h.distinct = x->distinct; h.generated = x->generated; h.max_front = x->max_front;
    h.cur_base = s.cur_base; h.n_cur = s.n_cur; h.parents_n = s.cur_base + s.n_cur;
    h.finished = x->finished; h.viol_mask = s.viol_mask; h.viol_in_model = s.viol_in_model;
    h.viol_inst = s.viol_inst; h.viol_parent = s.viol_parent; h.viol_child = s.viol_child;
    const std::string tmp = ckpt_path(prefix, s.id) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { failed = 1; break; }
    DevCounters c;
    bool ok = write_all(f, &h, sizeof h) && dev_to_file(f, s.table, 8ull << x->tlog2, buf) &&
              (!s.sent || dev_to_file(f, s.sent, 8ull << x->slog2, buf)) &&
              dev_to_file(f, s.parents, 8 * h.parents_n, buf) &&
              ring_to_file(f, cur_ring(x, s), x->L.W, s.n_cur, buf) &&
              hipMemcpy(&c, s.ctr, sizeof c, hipMemcpyDeviceToHost) == hipSuccess &&
              write_all(f, c.cover, sizeof c.cover);
    ok = ok && fflush(f) == 0 && fsync(fileno(f)) == 0;
    ok = fclose(f) == 0 && ok;
    if (!ok) { failed = 1; break; }
  }
  if (int rc = allreduce_u64(x, &failed, 1, 1)) return rc;
  if (failed) {
    for (auto& s : x->sh) (void)remove((ckpt_path(prefix, s.id) + ".tmp").c_str());
    return RTLA_E_ARG;
  }
  // the renames are agreed on too: every rank reports the same outcome
  uint64_t renamed_bad = 0;
  for (auto& s : x->sh) {
    const std::string path = ckpt_path(prefix, s.id);
    if (rename((path + ".tmp").c_str(), path.c_str()) != 0) renamed_bad = 1;
  }
  if (int rc = allreduce_u64(x, &renamed_bad, 1, 1)) return rc;
  if (renamed_bad) {
    fprintf(stderr, "rtla: checkpoint %s: a shard file could not be renamed into place "
                    "(the checkpoint mixes generations; recover will refuse it)\n", prefix);
    return RTLA_E_ARG;
  }
  return RTLA_OK;
}

extern "C" int rtla_recover(rtla_ctx* x, const char* prefix) {
  if (!x || !prefix) return RTLA_E_ARG;
  if (x->cfg.mode == RTLA_MODE_DEDUP) return RTLA_E_STATE;
  std::vector<char> buf(64 << 20);
  int level = -1;
  int err = hipSetDevice(x->device) != hipSuccess ? RTLA_E_HIP : RTLA_OK;  // the first local failure
  for (auto& s : x->sh) {
    if (err) break;
    FILE* f = fopen(ckpt_path(prefix, s.id).c_str(), "rb");
    if (!f) { err = RTLA_E_ARG; break; }
    CkptHeader h;
    bool ok = read_all(f, &h, sizeof h) && memcmp(h.magic, "RTLACKP1", 8) == 0 && h.abi == RTLA_ABI_VERSION &&
              h.nshard == x->nshard && h.shard == s.id && h.W == x->L.W && h.tlog2 == x->tlog2 &&
              memcmp(&h.cfg, &x->cfg, offsetof(rtla_cfg, fpset_log2)) == 0 && h.parents_n <= s.parents_cap &&
              h.n_cur <= x->front_cap && (level < 0 || level == h.level);
    DevCounters c;
    memset(&c, 0, sizeof c);
    ok = ok && file_to_dev(f, s.table, 8ull << x->tlog2, buf) &&
         (!s.sent || file_to_dev(f, s.sent, 8ull << x->slog2, buf)) &&
         file_to_dev(f, s.parents, 8 * h.parents_n, buf) &&
         file_to_dev(f, s.arena, 4ull * x->L.W * h.n_cur, buf) && read_all(f, c.cover, sizeof c.cover);
    fclose(f);
    if (!ok) { err = RTLA_E_STATE; break; }
    if (hipMemcpy(s.ctr, &c, sizeof c, hipMemcpyHostToDevice) != hipSuccess) { err = RTLA_E_HIP; break; }
    level = h.level;
    s.cur_start = 0; s.cur_base = h.cur_base; s.n_cur = h.n_cur;
    s.viol_mask = h.viol_mask; s.viol_in_model = h.viol_in_model; s.viol_inst = h.viol_inst;
    s.viol_parent = h.viol_parent; s.viol_child = h.viol_child;
    x->level = h.level; x->distinct = h.distinct; x->generated = h.generated; x->max_front = h.max_front;
    x->finished = h.finished != 0;
  }
  if (x->world > 1) {  // every rank must resume from the same level of the same search
    uint64_t v[7] = {(uint64_t)x->level, x->distinct, x->generated, ~(uint64_t)x->level, ~x->distinct, ~x->generated,
                     err ? 1ull : 0ull};
    if (int rc = allreduce_u64(x, v, 7, 1)) return rc;
    if (err) return err;
    if (v[6]) {
      fprintf(stderr, "rtla: recover failed on another rank\n");
      return RTLA_E_STATE;
    }
    if (v[0] != ~v[3] || v[1] != ~v[4] || v[2] != ~v[5]) {
      fprintf(stderr, "rtla: checkpoint files of different ranks are from different levels\n");
      return RTLA_E_STATE;
    }
  } else if (err) {
    return err;
  }
  x->roots.assign(x->L.W, 0);
  row_init(x->L, x->roots.data());
  x->seeded = false;
  x->inited = true;
  x->sim.viol = false;
  return RTLA_OK;
}
