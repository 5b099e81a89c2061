// hostmodel.cpp -- TEST INFRASTRUCTURE: the product's model code
// (raft-tla_amd/csrc/rtla_model.h, written once for host and device)
// compiled for the host, so the CPU test suite can check the semantics the
// kernels evaluate -- successor generation, incremental fingerprints, row
// building -- against the oracles without a GPU.  The product never runs
// this: its only expansion path is the HIP level kernel (librtla.so).
//
// hm_expand mirrors the level kernel's per-successor work: compute_delta on
// the parent row, the fingerprint derived incrementally (parent fp +
// allLogs' change + delta_fp), the child row materialised from the patches.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "rtla_audit.h"
#include "rtla_device.h"
#include "rtla_model.h"
#include "rtla_plan.h"

using namespace rtla;

extern "C" {

// layout of a model (K, E: bag slots, election records); 0 on success
int hm_layout(int n, int v, int t, int l, int c, int m, int k, int e, int inv, int sym, int* words) {
  Layout L;
  if (make_layout(&L, n, v, t, l, c, m, k, e, inv) != 0) return -1;
  *words = L.W;
  (void)sym;
  return 0;
}

// Every enabled successor of each input row: out rows, info[k] = its successor
// record (successor_info, rtla_device.h).  Returns the count, or -1 if cap is
// too small, -2 on a row-capacity error, -3 on a spec error.
long hm_expand(int n, int v, int t, int l, int c, int m, int k, int e, int inv, const uint32_t* rows, size_t nrows,
               uint32_t* out, uint64_t* info, size_t cap) {
  Layout L;
  if (make_layout(&L, n, v, t, l, c, m, k, e, inv) != 0) return -4;
  const int W = L.W;
  size_t cnt = 0;
  std::vector<uint32_t> pall(L.all_words + 1);
  for (size_t s = 0; s < nrows; s++) {
    const uint32_t* row = rows + s * W;
    const FP pfp = fp_add(row_fp(row), alllogs_delta<0>(L, row, pall.data()));
    for (int inst = 0; inst < L.fam[F_COUNT]; inst++) {
      Delta d;
      compute_delta<0>(L, row, inst, d);
      if (!d.enabled) continue;
      if (d.err) return d.err == 1 ? -3 : -2;
      if (cnt >= cap) return -1;
      const FP cfp = fp_add(pfp, delta_fp<0>(L, row, d));
      materialize<0>(L, row, d, pall.data(), cfp, out + cnt * W);
      info[cnt] = successor_info(s, d.in_model, d.sub, inst);
      cnt++;
    }
  }
  return (long)cnt;
}

// The three 64-bit records (rtla_device.h): kind 0 parent record (shard, index,
// instance), 1 successor record (input, in_model, sub, instance), 2 outbox ref
// (parent, instance).  hm_record_fields: the accessors' view of r, in out[0..3].
uint64_t hm_record(int kind, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  return kind == 0 ? parent_record(a, b, c) : kind == 1 ? successor_info(a, b != 0, c, d) : outbox_ref(a, b);
}
void hm_record_fields(int kind, uint64_t r, uint64_t* out) {
  out[0] = kind == 0 ? parent_shard(r) : kind == 1 ? successor_input(r) : outbox_parent(r);
  out[1] = kind == 0 ? parent_index(r) : kind == 1 ? (uint64_t)successor_label(r) : (uint64_t)outbox_inst(r);
  out[2] = kind == 0 ? (uint64_t)parent_inst(r) : kind == 1 ? (uint64_t)successor_inst(r) : 0;
}

// The violation key of the passes over rows (rtla_audit.h).  hm_audit_key_fields: the accessors' view of key,
// in out[0..3] (index, instance, in_model, mask).
uint64_t hm_audit_key(uint64_t index, int inst, int in_model, int mask) { return audit_key(index, inst, in_model, mask); }
void hm_audit_key_fields(uint64_t key, uint64_t* out) {
  out[0] = audit_key_index(key);
  out[1] = (uint64_t)audit_key_inst(key);
  out[2] = (uint64_t)audit_key_in_model(key);
  out[3] = (uint64_t)audit_key_mask(key);
}

// Fingerprint of a row from scratch.
int hm_fingerprint(int n, int v, int t, int l, int c, int m, int k, int e, int inv, const uint32_t* row, uint64_t* out) {
  Layout L;
  if (make_layout(&L, n, v, t, l, c, m, k, e, inv) != 0) return -4;
  const FP f = row_fingerprint(L, row);
  out[0] = f.a;
  out[1] = f.b;
  return 0;
}

// The multi-shard driver's level-end plans (rtla_plan.h).  Moves come back as
// 5 words each; the count, -1 if the plan reports "full" (rehome), -2 if cap
// is too small.  n (rehome) / m (rebalance): the counts after the moves.
long hm_plan_rehome(int G, uint64_t rows_cap, const uint64_t* expm, const uint64_t* room, uint64_t* n, uint64_t* out,
                    size_t cap) {
  std::vector<uint64_t> nv(n, n + G);
  std::vector<RehomeMove> mv;
  const bool ok = plan_rehome(G, rows_cap, expm, room, nv, mv);
  memcpy(n, nv.data(), 8 * (size_t)G);
  if (!ok) return -1;
  if (mv.size() > cap) return -2;
  for (size_t k = 0; k < mv.size(); k++) {
    const uint64_t v[5] = {(uint64_t)mv[k].a, (uint64_t)mv[k].b, (uint64_t)mv[k].dst, mv[k].base, mv[k].cnt};
    memcpy(out + 5 * k, v, sizeof v);
  }
  return (long)mv.size();
}

long hm_plan_rebalance(int G, const uint64_t* n, uint64_t* m, uint64_t* out, size_t cap) {
  std::vector<uint64_t> mv_after;
  const std::vector<RebalanceMove> mv = plan_rebalance(G, std::vector<uint64_t>(n, n + G), mv_after);
  memcpy(m, mv_after.data(), 8 * (size_t)G);
  if (mv.size() > cap) return -2;
  for (size_t k = 0; k < mv.size(); k++) {
    const uint64_t v[5] = {(uint64_t)mv[k].a, (uint64_t)mv[k].b, mv[k].first, mv[k].base, mv[k].cnt};
    memcpy(out + 5 * k, v, sizeof v);
  }
  return (long)mv.size();
}

}  // extern "C"
