// rtla_klevel.h -- the level kernel k_expand_compact, its private helpers and
// its launcher launch_compact (shared device helpers: rtla_kdev.h).
//
// The level kernel is a template over the server count, the group size, the
// compiled-in layout and SYMMETRY; its instantiations are spread over several
// translation units (rtla_kspec_*.hip, rtla_ksym_*.hip, rtla_kgeneric_*.hip)
// that compile in parallel, each exporting one launcher (launch_compact_*,
// rtla_launch.h).  Only they and rtla_kernels.hip (the dispatch, the LDS
// sizes) include this header.
#pragma once
#include "rtla_kdev.h"

namespace {

// a[j] += v for a run-time j (selects)
template <int NS>
__device__ __forceinline__ void add_at(uint32_t* a, uint32_t j, uint32_t v) {
#pragma unroll
  for (int k = 0; k < NS; k++)
    if ((uint32_t)k == j) a[k] += v;
}
// The orbit key in steps of one image (key_chunk's continuations): images
// [k, k + 1) of the successor parent + d -- or [k, |C(s)|) when `all` --
// folded into best (the least image fingerprint so far).  Returns the next
// image's index, or -1 once best is the least image (the key is then
// orbit_key_finish(best) + fp(allLogs'), as sym_key's).
// The successor's signatures are PATCHED from the parent's parts (psg[w * S],
// w < 3 * NS: srv_sig, sent and received message sums per server, computed
// once per parent row): the changed server's local part is recomputed, each
// bag write moves its old slot's share out of and its new slot's share into
// the sums -- no pass over the successor's bag and records.  The same
// signatures, hence the same key, as sym_rank's.
template <int NS, int S, class P>
__device__ __forceinline__ int successor_orbit_step_sig(const Layout& L, P prow, const DeltaT<NS>& d,
                                                        const uint32_t* psg, int k, bool all, FP& best) {
  return with_successor<NS>(L, prow, d, [&](auto rec_of, int nmsg, auto slot_of, int nelec, auto elec_of) {
    uint32_t ms[NS], mr[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) {
      ms[j] = psg[(NS + j) * S];
      mr[j] = psg[(2 * NS + j) * S];
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
      if (q >= d.nops) continue;
      const uint64_t o = d.op_old[q], v = d.op_new[q];
      if (o) {
        const uint32_t c = slot_sig_sent(L, o);
        add_at<NS>(ms, slot_src(L, o), 0u - c);
        add_at<NS>(mr, slot_dst(L, o), 0u - slot_sig_recv(c));
      }
      if (v) {
        const uint32_t c = slot_sig_sent(L, v);
        add_at<NS>(ms, slot_src(L, v), c);
        add_at<NS>(mr, slot_dst(L, v), slot_sig_recv(c));
      }
    }
    const uint32_t lsrv = d.srv >= 0 ? srv_sig<NS>(d.srv, d.rec) : 0u;
    uint64_t sig[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) sig[i] = sig_of(i == d.srv ? lsrv : psg[i * S], ms[i], mr[i]);
    const SymRank r = sym_rank_from<NS>(L, sig, rec_of, nmsg, slot_of, nelec, elec_of);
    const int k1 = all ? r.ncomb : min(k + 1, r.ncomb);
    for (int j = k; j < k1; j++) {
      const FP f = sym_image_fp<NS>(L, rec_of, nmsg, slot_of, nelec, elec_of, r, j);
      if (fp_less(f, best)) best = f;
    }
    return k1 < r.ncomb ? k1 : -1;
  });
}

}  // namespace

// ------------------------------------------------------------------------
// k_expand_compact: the single-shard BFS level kernel with work compaction.
//
// A wave owns 64 consecutive frontier rows in LDS.  Each lane first
// computes, for its own state, the bit mask of action instances whose
// enabling guard holds (the guards of raft.tla's actions, below).  The wave
// then lists the (state, instance) pairs in instance-major order -- so
// consecutive pairs belong to the same family of Next -- and evaluates them
// 64 at a time, one pair per lane.  Every lane of a chunk does useful work
// and a chunk spans at most a few families, instead of sweeping all ~45
// instances with most lanes idle.  Fingerprint-set CAS of chunk c are
// resolved after chunk c+1 is computed; new states go to a per-wave LDS list
// and reserve next-frontier slots 64+ at a time (one atomic per flush).
namespace {

constexpr int RING = 128;   // pair ring (u16: state lane << 8 | instance - window base)
constexpr int NEWCAP = 512; // new-state list (u16: state lane << 8 | instance)
// The list is built into rows at the group's end; a group that finds more
// new states (early levels) flushes it when it holds more than this many --
// after which one chunk (<= 64) and a drain (<= 2 x 64) may still add
// entries before the flush.
constexpr int NEWFLUSH = NEWCAP - 3 * 64;


// Per-wave LDS of k_expand_compact (16-byte aligned pieces first):
// per-state fingerprint with allLogs' applied (GROUP FPs) | SYMMETRY: the
// fingerprint of each state's allLogs' (GROUP FPs) | per-owner (base, used)
// of the open outbox chunk | pending new states (NEWCAP u16 entries) |
// GROUP rows | allLogs' words of each state | pair ring | SYMMETRY: key ring,
// key continuations (64 least-image-so-far FPs, 64 entries).
// (The outbox state exists only in the MULTI kernels: one shard's tile then
// stays small enough for 12 one-wave blocks per CU on configs[1]'s 372-byte rows.)
__host__ __device__ constexpr int compact_lds_words(int W, int AW, int GROUP, bool sym, bool multi) {
  return (4 * GROUP * (sym ? 2 : 1) + (multi ? 4 * SHARD_MAX : 0) + NEWCAP / 2 + GROUP * W + GROUP * AW +
          RING / 2 * (sym ? 2 : 1) + (sym ? 5 * 64 + 3 * NMAX * GROUP : 0) + 3) & ~3;
}

// bits << off into a 64-bit window mask (off may be negative or >= 64)
__device__ __forceinline__ unsigned long long win_bits(unsigned long long bits, int off) {
  if (off >= 64 || off <= -64) return 0ull;
  return off >= 0 ? bits << off : bits >> (-off);
}

// Instances [wb, wb+64) whose enabling guard holds in `row`.  A superset is
// safe (compute_delta re-checks every guard); a subset would lose states.
// dup = false: without DuplicateMessage (counted apart, see dup_counted).
template <int NS>
__device__ __forceinline__ unsigned long long cand_mask(const Layout& L, const uint32_t* row, int nmsg, int wb,
                                                        bool dup = true) {
  constexpr int N = NS;
  unsigned long long rv = 0, bl = 0, ldr = 0, tmo = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const uint32_t w0 = srv_w0(L, row, i);
    const uint32_t role = s_role(w0);
    if (role == FOLLOWER || role == CANDIDATE) tmo |= 1ull << i;          // Timeout :178-181
    if (role == CANDIDATE) {
      rv |= (unsigned long long)(~s_vresp(w0) & ((1u << N) - 1u)) << (i * N);  // RequestVote :190-192
      if (__builtin_popcount(s_vgrant(w0)) * 2 > N) bl |= 1ull << i;     // BecomeLeader :229-231
    }
    if (role == LEADER) ldr |= 1ull << i;                                 // :204-206, :246-248, :259-260
  }
  unsigned long long ae = 0, cr = 0;
#pragma unroll
  for (int i = 0; i < N; i++)
    if (ldr >> i & 1ull) {
      ae |= (((1ull << N) - 1ull) & ~(1ull << i)) << (i * N);             // AppendEntries i /= j
      cr |= ((1ull << L.V) - 1ull) << (i * L.V);                           // ClientRequest(i, v)
    }
  const unsigned long long bag = nmsg >= 64 ? ~0ull : ((1ull << nmsg) - 1ull);
  unsigned long long m = 0;
  m |= win_bits((1ull << N) - 1ull, L.fam[F_RESTART] - wb);               // Restart: always
  m |= win_bits(tmo, L.fam[F_TIMEOUT] - wb);
  m |= win_bits(rv, L.fam[F_REQUESTVOTE] - wb);
  m |= win_bits(bl, L.fam[F_BECOMELEADER] - wb);
  m |= win_bits(cr, L.fam[F_CLIENTREQUEST] - wb);
  m |= win_bits(ldr, L.fam[F_ADVANCECOMMIT] - wb);
  m |= win_bits(ae, L.fam[F_APPENDENTRIES] - wb);
  m |= win_bits(bag, L.fam[F_RECEIVE] - wb);
  if (dup) m |= win_bits(bag, L.fam[F_DUPLICATE] - wb);
  m |= win_bits(bag, L.fam[F_DROP] - wb);
  return m;
}

// Zero records (fp 0:0, skipped by k_insert_remote) in outbox slots [from, to) of owner o.
__device__ __forceinline__ void outbox_holes(const ShardBox& box, int o, unsigned long long from,
                                             unsigned long long to, int lane) {
  to = min(to, box.cap);
  for (unsigned long long j = from + lane; j < to; j += 64) {
    const unsigned long long k = (unsigned long long)o * box.cap + j;
    box.send_fp[2 * k] = 0ull;
    box.send_fp[2 * k + 1] = 0ull;
  }
}

// Home slot of a key in a table of 2^lg slots (lg = 0: no table, slot 0).
__device__ __forceinline__ unsigned long long home_slot(const FP& key, int lg) {
  return lg ? key.a >> (64 - lg) : 0ull;
}

}  // namespace

#ifndef RTLA_COMPACT_WAVES_PER_EU
#define RTLA_COMPACT_WAVES_PER_EU 3  // 168 VGPRs (3 waves/SIMD); spills per instantiation: profiles/r04_*/resource_usage.txt
#endif
#ifndef RTLA_SYM_WAVES_PER_EU
#define RTLA_SYM_WAVES_PER_EU 4      // SYMMETRY, the key pass a call of its own (key_one): 128 VGPRs (configs[3]:
                                     // 311.5 ms, 16-state groups) beat 168 (343 ms) and 102 (414 ms)
#endif

namespace {
// One key_chunk lane as a function of its own: the successor's Delta, then
// successor_orbit_step_sig from image k with the least image so far best0.
// next >= 0: f is the least image so far and image `next` is due; next ==
// -1: f is the orbit key; next == -2: the instance is not enabled.  NOT
// inlined, so that its registers are allocated apart from the level
// kernel's: inlined, the continuation bookkeeping spilled the kernel to 712
// VGPRs (750 ms per configs[3] step); as a call, 343 ms against 355 ms for
// the inlined all-images key pass (profiles/r04_v4).
struct KeyStep {
  FP f;
  int next;
};
template <int NS, Layout LC, int S>
__device__ __noinline__ KeyStep key_one(const Layout& Lrt, const uint32_t* prow, const uint32_t* psg, int inst, int k,
                                        bool all, FP best0, FP afp) {
  const Layout& L = pick_layout<LC>(Lrt);
  DeltaT<NS> d;
  d.enabled = 0;
  compute_delta<NS>(L, prow, inst, d);
  KeyStep r{FP{0, 0}, -1};
  if (!d.enabled) {
    r.next = -2;
    return r;
  }
  FP best = best0;
  r.next = successor_orbit_step_sig<NS, S>(L, prow, d, psg, k, all, best);
  r.f = r.next < 0 ? fp_add(orbit_key_finish(best), afp) : best;
  return r;
}

// Entry k of a packed server / election record (at most PACKW words) for a
// run-time k, as a select chain: a run-time index would move the record to scratch.
__device__ __forceinline__ uint32_t pack_word(const uint32_t* a, int k) {
  uint32_t v = a[0];
#pragma unroll
  for (int j = 1; j < PACKW; j++)
    if (k == j) v = a[j];
  return v;
}
// Word w of the successor row parent + d (ne: its election records): what
// child_write (rtla_model.h) puts there, else the parent's word.  With a
// compiled-in layout and a constant w every test but the compares against
// d.srv, ne - 1 and the op slots folds away.
template <class P, class R, int NR>
__device__ __forceinline__ uint32_t child_word(const Layout& L, P prow, const DeltaT<NR>& d, const uint32_t* spk,
                                               const uint32_t* epk, R all_new, FP fp, int ne, int w) {
  if (w < 4)
    return w == 0 ? (uint32_t)fp.a : w == 1 ? (uint32_t)(fp.a >> 32) : w == 2 ? (uint32_t)fp.b : (uint32_t)(fp.b >> 32);
  if (w == L.off_hdr) return (uint32_t)d.nmsg | (uint32_t)ne << 8;
  if (w >= L.off_all && w < L.off_elec) return all_new[w - L.off_all];
  uint32_t v = prow[w];
  if (w < L.off_all) {  // a server record
    const int i = (w - L.off_srv) / L.srv_w;
    if (d.srv == i) v = pack_word(spk, w - L.off_srv - i * L.srv_w);
  } else if (w < L.off_bag) {  // an election record
    const int e = (w - L.off_elec) / L.elec_w;
    if (d.elec && e == ne - 1) v = pack_word(epk, w - L.off_elec - e * L.elec_w);
  } else {  // a bag slot (or the padding word behind the bag: no op names it); a later op on a slot wins
    const int q = (w - L.off_bag) / L.slot_w;
    const bool hi = w - L.off_bag - q * L.slot_w != 0;
#pragma unroll
    for (int o = 0; o < 3; o++)
      if (o < d.nops && d.op_slot[o] == q) v = hi ? (uint32_t)(d.op_new[o] >> 32) : (uint32_t)d.op_new[o];
  }
  return v;
}
// The successor row parent + d, assembled word by word by its own lane and
// stored to dst (its W words; 4-byte aligned) with 16-byte stores: every
// word written exactly once, by one lane, no copy of the parent row first.
struct __attribute__((packed, aligned(4))) RowWords4 {
  uint32_t v[4];
};
// (FIXED: a compiled-in layout -- the loop over the words unrolls in full.)
template <bool FIXED, class P, class R, int NR>
__device__ __forceinline__ void child_store(const Layout& L, P prow, const DeltaT<NR>& d, const uint32_t* spk,
                                            const uint32_t* epk, R all_new, FP fp, uint32_t* dst) {
  const int ne = row_nelec(L, prow) + (d.elec ? 1 : 0);
  auto store4 = [&](int w) {
    RowWords4 t;
#pragma unroll
    for (int k = 0; k < 4; k++) t.v[k] = child_word(L, prow, d, spk, epk, all_new, fp, ne, w + k);
    *reinterpret_cast<RowWords4*>(dst + w) = t;
  };
  int w = 0;
  if constexpr (FIXED) {
#pragma unroll
    for (; w + 4 <= L.W; w += 4) store4(w);
#pragma unroll
    for (; w < L.W; w++) dst[w] = child_word(L, prow, d, spk, epk, all_new, fp, ne, w);
  } else {
    for (; w + 4 <= L.W; w += 4) store4(w);
    for (; w < L.W; w++) dst[w] = child_word(L, prow, d, spk, epk, all_new, fp, ne, w);
  }
}

// One build_all lane as a function of its own (SYMMETRY kernels): the new
// state's full Delta, fingerprint and invariants, then its row (child_store;
// dst = nullptr: none).  NOT inlined for the same reason as key_one: at the SYMMETRY
// kernel's 128 VGPRs the inlined build pass is one of the two big spillers.
struct BuildOut {
  int bad, sub, in_model;
};
template <int NS, Layout LC, int GROUP>
__device__ __noinline__ BuildOut build_one(const Layout& Lrt, const uint32_t* prow, int inst, FP qfp,
                                           const uint32_t* pall_p, uint32_t* dst) {
  const Layout& L = pick_layout<LC>(Lrt);
  DeltaT<NS> d;
  d.enabled = 0;
  compute_delta<NS>(L, prow, inst, d);
  const FP cfp = fp_add(qfp, delta_fp<NS>(L, prow, d));
  BuildOut o{check_invariants_v<NS>(L, prow, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]), d.sub, d.in_model};
  uint32_t spk[PACKW], epk[PACKW];
  child_pack(L, d, spk, epk);
  if (dst) child_store<LC.N != 0>(L, prow, d, spk, epk, StridedWords<GROUP>{const_cast<uint32_t*>(pall_p)}, cfp, dst);
  return o;
}

}  // namespace

// RTLA_STAMPS (diagnostic builds only): per-wave cycle counts of the level
// kernel's phases from s_memtime (each stamp waits for the wave's LDS
// operations in flight: a perturbation, fine for shares) summed into
// DevCounters::stamp.
#ifdef RTLA_STAMPS
#define RTLA_STAMP_DECL                                                   \
  unsigned long long st_prev_ = __builtin_amdgcn_s_memtime();              \
  unsigned long long st_acc_[RTLA_NSTAMP] = {};
#define STAMP(k)                                                             \
  do {                                                                       \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();              \
    st_acc_[k] += t_ - st_prev_;                                             \
    st_prev_ = t_;                                                           \
  } while (0)
#define RTLA_STAMP_FLUSH(ctr, lane)                                          \
  if ((lane) == 0)                                                           \
    for (int k_ = 0; k_ < RTLA_NSTAMP; k_++) atomicAdd(&(ctr)->stamp[k_], st_acc_[k_]);
#else
#define RTLA_STAMP_DECL
#define STAMP(k)
#define RTLA_STAMP_FLUSH(ctr, lane)
#endif

// GROUP: frontier states per wave-group (64, or 32 for wide rows: halves the
// LDS tile so more waves fit a CU).  LC: compiled-in layout (Layout{} = use
// the run-time argument Lrt).  SYM: SYMMETRY Permutations(Server) -- the
// successors are probed by their orbit key, computed in a pass of its own
// (key_chunk), instead of their fingerprint; rows keep the states themselves.
// Waves per SIMD the level kernel's registers are budgeted for: narrow
// compiled-in rows (<= 32 words: the exhaust model's 84 B) fit 4 (128
// VGPRs; its 74 levels 1259 -> 1158 ms; 5 waves: 1605 ms), wider ones 3 (at 4: configs[1]
// 197.9 -> 215.6 ms, configs[2] 90.0 -> 100.0 ms, configs[0]'s 37-word rows
// 300.9 -> 328.0 ms; profiles/r04_v4/waves{3,4}_*).
#ifndef RTLA_NARROW_W
#define RTLA_NARROW_W 32  // rows of at most this many words get RTLA_NARROW_WAVES waves/SIMD
#endif
#ifndef RTLA_NARROW_WAVES
#define RTLA_NARROW_WAVES 4
#endif
constexpr int compact_waves(const Layout& L, bool sym) {
  return sym ? RTLA_SYM_WAVES_PER_EU
             : (L.N != 0 && L.W <= RTLA_NARROW_W ? RTLA_NARROW_WAVES : RTLA_COMPACT_WAVES_PER_EU);
}
template <int NS, bool MULTI, int GROUP, Layout LC, bool SYM>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(compact_waves(LC, SYM))))
k_expand_compact(Layout Lrt, Ring cur, unsigned long long s_begin, unsigned long long s_end,
                 unsigned long long cur_base, Ring next, unsigned long long* __restrict__ parents,
                 unsigned long long next_base, unsigned long long next_cap, unsigned long long* table,
                 unsigned long long* sent, int tlog2, DevCounters* ctr, ShardBox box, int xflags) {
  const Layout& L = pick_layout<LC>(Lrt);
  const int me = box.me;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ unsigned int cov[2 * COVER_CODES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int W = L.W, AW = L.all_words;
  uint32_t* wl = lds + wave * compact_lds_words(W, AW, GROUP, SYM, MULTI);
  FP* pfpl = reinterpret_cast<FP*>(wl);  // [state lane]: its fingerprint + the allLogs' change (raft.tla:465)
  FP* afpl = pfpl + GROUP;               // SYM [state lane]: fingerprint of its allLogs'
  unsigned long long* obox =             // [o] base of the open chunk, [SHARD_MAX + o] used
      reinterpret_cast<unsigned long long*>(wl + 4 * GROUP * (SYM ? 2 : 1));
  uint16_t* newl = reinterpret_cast<uint16_t*>(obox + (MULTI ? 2 * SHARD_MAX : 0));
  uint32_t* rows = reinterpret_cast<uint32_t*>(newl + NEWCAP);
  uint32_t* pall = rows + GROUP * W;  // allLogs' words of state lane l: pall[l + w * GROUP]
  const StridedWords<GROUP> pall_mine{pall + (lane & (GROUP - 1))};
  uint16_t* ring = reinterpret_cast<uint16_t*>(pall + GROUP * AW);
  // SYMMETRY: successors that need an orbit key (in-model, not the parent),
  // queued by the evaluation pass and keyed 64 at a time (key_chunk)
  uint16_t* kring = ring + RING;
  int kpos = 0, kdone = 0;
  // SYMMETRY: successors whose orbit key needs more images than key_chunk
  // computes per pass (one): entry (state lane << 8 | instance | next image
  // << 16) and the least image fingerprint so far; taken first by the next
  // key chunk (ccount of them, uniform)
  FP* cbest = reinterpret_cast<FP*>(kring + (SYM ? RING : 0));
  uint32_t* cent = reinterpret_cast<uint32_t*>(cbest + (SYM ? 64 : 0));
  int ccount = 0;
  // SYMMETRY: each tile row's signature parts (sym_sig_parts: srv_sig, sent
  // and received message sums per server), word w of row r at sigl[w * GROUP + r]
  uint32_t* sigl = cent + (SYM ? 64 : 0);
  if (MULTI) {
    if (lane < SHARD_MAX) {
      obox[lane] = ~0ull;
      obox[SHARD_MAX + lane] = OBOX_CHUNK;
    }
    wave_sync();
  }
  cover_zero(cov, 2 * COVER_CODES);

  unsigned my_gen = 0, my_probe = 0;
  unsigned my_dup = 0;  // DuplicateMessage successors counted, not evaluated (dup_counted)
#ifdef RTLA_COUNT_CAS
  unsigned my_cas = 0;
#endif
  const int ninst = L.fam[F_COUNT];
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  // DuplicateMessage successors counted, not evaluated (see the group loop)
  // (in the narrow-row kernels too since the round-6 pair ring: the exhaust
  // model 1120-1127 against 1142-1150 ms, profiles/r09_rowbuild/others_ab.txt)
  constexpr bool narrow = !SYM && LC.N != 0 && LC.W <= RTLA_NARROW_W;
  const bool dup_counted = L.C == 1 && !(xflags & (XF_ALL_SUCCESSORS | XF_NO_CHUNKS));
  // Receive pairs are grouped by message type in the pair ring (4 ballots per
  // instance) only for SYMMETRY and max copies > 1 (round 6,
  // profiles/r06_v2/pairring_ab.txt: ungrouped configs[1] 178.1 vs 179.7 ms,
  // configs[0] 257.0 vs 263.3, the exhaust model 1148 vs 1211; grouped
  // configs[2] 89.4 vs 91.2, configs[3] 288.7 vs 293.6)
  const bool recv_group = SYM || L.C > 1;
  // A chunk is cut at a family boundary once family_cut pairs are queued, so
  // that it holds one family and runs compute_delta specialised for it;
  // 64 = never: full chunks of mixed families (round 6 sweep,
  // profiles/r06_v2/pairring_ab.txt: 22 -> 64 takes configs[1] 178.3 -> 170.0
  // ms, configs[0] 258.6 -> 245.6, configs[2] 90.4 -> 87.3; the SYMMETRY
  // kernel is best at 40 (285.9 vs 287.1 / 291.6), the narrow-row exhaust
  // kernel at 22 (1145 vs 1153))
  constexpr int family_cut = narrow ? 22 : SYM ? 40 : 64;
  RTLA_STAMP_DECL
  // pending probe (issued by the previous chunk).  MULTI: a successor owned
  // by another shard probes this shard's SENT cache instead of the set --
  // a dedup hint, one slot per fingerprint (2^box.slog2 slots), overwritten
  // on a miss: a hit drops the copy (this shard sent it to its owner
  // already), a miss queues its (fingerprint, parent) record for the owner
  // and stores the key in the slot (a plain store, issued like the CAS of a
  // set insert and reported a chunk later).  Bounded work per probe, never
  // full; a slot overwritten by another key only costs a duplicate record,
  // which the owner deduplicates.
  bool pend = false;
  unsigned long long pold = 0;
  FP pf{0, 0};       // its fingerprint (home slot and owner derive from it)
  uint32_t pinfo = 0;  // its state lane << 16 | action instance
  // A probe whose home-slot load did not show its key issues ONE CAS -- at
  // the home slot if it read empty, else at the next slot (linear probing;
  // slots only ever go 0 -> key) -- together with the next chunk's loads,
  // and that CAS is resolved a chunk later: neither the insert nor the first
  // collision step waits for a round trip.  (MULTI, a successor another
  // shard owns: the sent-cache store instead, see above.)
  const bool async_cas = !(xflags & XF_CAS_ONLY);
  bool cpend = false;    // CAS set up by resolve(), issued by issue_cas()
  bool cflight = false;  // CAS in flight (result in cold)
  unsigned long long cold = 0, ckey = 0, cidx = 0;
  uint32_t cinfo = 0;
  // New states found so far whose rows are not built yet: newl[head, tail)
  // (mod NEWCAP) holds (state lane, instance); their parents are rows of the
  // current group (uniform counters).  They are built when the group's probes
  // have drained (build_all), so no probe or CAS state is live while the
  // rows are built.
  int head = 0, tail = 0;
  unsigned long long dedup_new = 0;  // XF_DEDUP_ONLY: new fingerprints (uniform)
  unsigned long long s0 = 0;  // first state of the current group

  // compute_delta over a chunk of lanes, specialised for its family when the
  // whole chunk holds one (D = DeltaFpT for the probe pass, DeltaT for the
  // row build and orbit keys)
  auto chunk_delta = [&](bool active, const uint32_t* prow, int inst, auto& d) {
    const int f0 = inst_family(L, __builtin_amdgcn_readfirstlane(inst));
    const bool one_family = __ballot(active && inst_family(L, inst) != f0) == 0ull;
    if (!one_family || (xflags & XF_GENERIC_DELTA)) {
      if (active) compute_delta<NS>(L, prow, inst, d);
    } else if (active) {
      switch (f0) {  // one family in the whole chunk: its code only
        case F_RESTART: compute_delta<NS, F_RESTART>(L, prow, inst, d); break;
        case F_TIMEOUT: compute_delta<NS, F_TIMEOUT>(L, prow, inst, d); break;
        case F_REQUESTVOTE: compute_delta<NS, F_REQUESTVOTE>(L, prow, inst, d); break;
        case F_BECOMELEADER: compute_delta<NS, F_BECOMELEADER>(L, prow, inst, d); break;
        case F_CLIENTREQUEST: compute_delta<NS, F_CLIENTREQUEST>(L, prow, inst, d); break;
        case F_ADVANCECOMMIT: compute_delta<NS, F_ADVANCECOMMIT>(L, prow, inst, d); break;
        case F_APPENDENTRIES: compute_delta<NS, F_APPENDENTRIES>(L, prow, inst, d); break;
        case F_RECEIVE: compute_delta<NS, F_RECEIVE>(L, prow, inst, d); break;
        case F_DUPLICATE: compute_delta<NS, F_DUPLICATE>(L, prow, inst, d); break;
        default: compute_delta<NS, F_DROP>(L, prow, inst, d); break;
      }
    }
  };
  // Coverage tally of one pass (base = cov: generated, cov + COVER_CODES:
  // distinct), aggregated over equal codes: the lanes that share the first
  // counting lane's code cost one atomic together.
  auto cover_add = [&](unsigned* base, bool on, int inst, int sub) {
    if (xflags & XF_NO_COVER) return;
    const int code = on ? cover_code(L, inst, sub) : -1;
    const unsigned long long m = __ballot(on);
    if (m) {
      const int c0 = __shfl(code, __builtin_ctzll(m));
      const bool same = on && code == c0;
      const int n0 = __popcll(__ballot(same));
      if (lane == 0) atomicAdd(&base[c0], (unsigned)n0);
      if (on && !same) atomicAdd(&base[code], 1u);
    }
  };
  // Build the rows of every pending new state (probes drained), one
  // next-level slot reservation for all of them (slots past next_cap are
  // dropped and flagged: the level is then reported incomplete):
  // per batch of 64, one state per lane:
  //  (1) its full Delta (compute_delta with slot bookkeeping; the probe pass
  //      only folded it into a hash), fingerprint, invariants and distinct
  //      coverage;
  //  (2) its row, assembled by the lane itself from the parent row in LDS
  //      and the Delta (child_store) and stored with 16-byte stores; the
  //      rows of a batch are contiguous, so its lines fill within the batch.
  // Every word is stored once and nothing here waits for a store.
  // The narrow-row kernels (rows of at most RTLA_NARROW_W words, 4 waves per
  // SIMD: the exhaust model) keep the earlier form instead -- the wave copies
  // every parent row to its child's slot with coalesced stores, waits for the
  // copies, and each lane stores the words in which its child differs on top
  // (child_write): with 21-word rows and few new states per group the copy is
  // a handful of wave-wide steps, and the row per lane measured 1185-1225
  // against 1142-1150 ms there (profiles/r09_rowbuild/others_ab.txt).
  // No separate row-building kernel: no parent-record read, no parent-row
  // gather, no second launch.
  auto build_all = [&]() {
    const int ntot = tail - head;  // uniform
    if (ntot == 0) return;
    // (reserve_rows and the record functions of rtla_device.h, spelled out: calling them here changes the
    // kernel's register allocation -- spilled VGPRs of every instantiation, profiles/r08_kdev)
    unsigned long long obase = 0;
    if (lane == 0) obase = atomicAdd(&ctr->next_count, (unsigned long long)ntot);
    obase = shfl0_u64(obase);
    if (obase + ntot > next_cap && lane == 0) set_flag(ctr, FLAG_FRONTIER_FULL);
    const int nrows = obase >= next_cap ? 0 : (int)min<unsigned long long>((unsigned long long)ntot, next_cap - obase);
    const bool rows_on = !(xflags & XF_NO_MATERIALIZE) && RTLA_IDX_OK(ctr, obase + nrows, ctr->cap_next + 1);
    const unsigned long long p0 = ring_idx(next, obase);
    const int n1 = (int)min<unsigned long long>(next.cap - p0, (unsigned long long)nrows) * W;  // words before the wrap
    uint32_t* d1 = next.base + p0 * (unsigned long long)W;
    // child c's row (a row never straddles the arena's end: n1 is whole rows)
    auto row_at = [&](int c) { return c * W < n1 ? d1 + c * W : next.base + (c * W - n1); };
    // narrow rows: for child rows [rb, re), word i of the run, lane-contiguous
    auto copy_rows = [&](int rb, int re) {
      const int nwords = re * W;
      int r = rb, w = lane;
      while (w >= W) { w -= W; r++; }
      for (int i0 = rb * W; i0 < nwords; i0 += 64) {
        const int i = i0 + lane;
        if (i < nwords) {
          const int sr = newl[(head + r) & (NEWCAP - 1)] >> 8;
          const uint32_t v = rows[sr * W + w];
          if (i < n1) d1[i] = v;
          else next.base[i - n1] = v;
        }
        w += 64;
        while (w >= W) { w -= W; r++; }
      }
    };
    if constexpr (narrow)
      if (rows_on) copy_rows(0, nrows);  // (all of them first: one pass of coalesced stores)
    for (int b = 0; b < ntot; b += 64) {
      const bool act = b + lane < ntot;
      const int e = act ? newl[(head + b + lane) & (NEWCAP - 1)] : 0;
      const int sl = e >> 8, inst = e & 255;
      const int child = b + lane;  // index in the run
      if constexpr (SYM) {  // the lane's work as a call of its own (build_one)
        BuildOut o{0, 0, 0};
        if (act)
          o = build_one<NS, LC, GROUP>(Lrt, rows + sl * W, inst, pfpl[sl], pall + sl,
                                      rows_on && child < nrows ? row_at(child) : nullptr);
        if (!(xflags & XF_ALL_SUCCESSORS) && claim_violation(ctr, o.bad, lane))
          record_violation(ctr, cur_base + s0 + sl, inst, 1, child < nrows ? next_base + obase + child : ~0ull);
        cover_add(cov + COVER_CODES, act, inst, o.sub);  // distinct coverage
        if (child < nrows && RTLA_IDX_OK(ctr, next_base + obase + child, ctr->cap_parents))
          parents[next_base + obase + child] =
              (xflags & XF_ALL_SUCCESSORS)
                  ? (cur_base + s0 + sl) << 32 | (unsigned long long)(o.in_model ? 1u : 0u) << 31 |
                        (unsigned long long)o.sub << 16 | (unsigned long long)inst
                  : (unsigned long long)me << 56 | (cur_base + s0 + sl) << 16 | (unsigned long long)inst;
        continue;
      }
      DeltaT<NS> d;
      d.enabled = 0;
      if (act) compute_delta<NS>(L, rows + sl * W, inst, d);
      const FP qfp = pfpl[sl];
      FP cfp{0, 0};
      int bad = 0;
      if (act) {
        const uint32_t* prow = rows + sl * W;
        cfp = fp_add(qfp, delta_fp<NS>(L, prow, d));
        bad = check_invariants_v<NS>(L, prow, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]);
      }
      if (!(xflags & XF_ALL_SUCCESSORS) && claim_violation(ctr, bad, lane))
        record_violation(ctr, cur_base + s0 + sl, inst, 1, child < nrows ? next_base + obase + child : ~0ull);
      cover_add(cov + COVER_CODES, act, inst, d.sub);  // distinct coverage
      uint32_t spk[PACKW], epk[PACKW];  // the changed records, packed
      if (act) child_pack(L, d, spk, epk);
      if constexpr (narrow) {
        if (rows_on) {  // the copies must land first (same words, other lanes)
          if (b == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (child < nrows) {
            const StridedWords<GROUP> pall_p{pall + sl};
            const int off = child * W;
            child_write(L, rows + sl * W, d, spk, epk, pall_p, cfp, [&](int w, uint32_t v) {
              const int i = off + w;
              if (i < n1) d1[i] = v;
              else next.base[i - n1] = v;
            });
          }
        }
      } else if (rows_on && child < nrows)  // (2)
        child_store<LC.N != 0>(L, rows + sl * W, d, spk, epk, StridedWords<GROUP>{pall + sl}, cfp, row_at(child));
      if (child < nrows && RTLA_IDX_OK(ctr, next_base + obase + child, ctr->cap_parents))
        parents[next_base + obase + child] =
            (xflags & XF_ALL_SUCCESSORS)
                ? (cur_base + s0 + sl) << 32 | (unsigned long long)(d.in_model ? 1u : 0u) << 31 |
                      (unsigned long long)d.sub << 16 | (unsigned long long)inst
                : (unsigned long long)me << 56 | (cur_base + s0 + sl) << 16 | (unsigned long long)inst;
    }
    head = tail;
  };
  auto issue_cas = [&]() {
#ifdef RTLA_COUNT_CAS
    if (cpend) my_cas++;
#endif
    if (cpend) cold = atomicCAS(&table[cidx], 0ull, ckey);
    cflight = cpend;
    cpend = false;
  };
  auto resolve = [&]() {
    bool isnew = false;
    // the state isnew refers to: its (tile row, instance)
    uint32_t ninfo = pinfo;
    const int powner = MULTI ? fp_owner(pf, box.nshard) : me;
    // MULTI: this chunk's successor another shard owns missed the sent cache:
    // its record is queued now (it has no CAS to wait for)
    bool rem = false;
    if (xflags & XF_ALL_SUCCESSORS) {  // every enabled successor is output (no seen set)
      isnew = pend;
    } else if (async_cas) {
      if (cflight) {  // the CAS issued one chunk ago
        if (cold == 0ull) isnew = true;
        else if (cold != ckey)  // rare: keep probing
          isnew = fpset_resolve(table, tlog2, ckey, cidx, cold, ctr);
      }
      ninfo = cinfo;
      cflight = false;
      if (pend) {  // this chunk's load -> seen, a CAS for the next issue, or (sent cache) a store and a record
        const unsigned long long key = pf.b | 1ull;
        if (MULTI && powner != me) {
          if (pold != key) {
            rem = true;
            if (box.slog2) sent[home_slot(pf, box.slog2)] = key;
          }
        } else if (pold != key) {
          const unsigned long long idx = pf.a >> (64 - tlog2);
          cidx = pold == 0ull ? idx : ((idx + 1ull) & ((1ull << tlog2) - 1ull));
          ckey = key;
          cinfo = pinfo;
          cpend = true;
        }
      }
    } else if (pend) {
      if (MULTI && powner != me) {  // the sent cache: a miss overwrites the slot
        rem = pold != (pf.b | 1ull);
        if (rem && box.slog2) sent[home_slot(pf, box.slog2)] = pf.b | 1ull;
      } else {
        const unsigned long long pidx = pf.a >> (64 - tlog2);
        isnew = (xflags & XF_CAS_ONLY) ? fpset_resolve(table, tlog2, pf.b | 1ull, pidx, pold, ctr)
                                       : fpset_resolve_loaded(table, tlog2, pf.b | 1ull, pidx, pold, ctr);
      }
    }
    if (MULTI) {  // records for other owners: all owners' outbox slots reserved in one step
      const uint32_t rinfo = pinfo;  // (the record is this chunk's successor)
      if (__ballot(rem)) {
        // lane o learns how many records owner o gets (ocnt), each record its
        // rank among its owner's (r)
        unsigned long long mym = 0;
        int ocnt = 0;
        for (int o = 0; o < box.nshard; o++) {
          const unsigned long long m = __ballot(rem && powner == o);
          if (powner == o) mym = m;
          if (lane == o) ocnt = __popcll(m);
        }
        // lane o keeps owner o's open chunk of OBOX_CHUNK slots (obox[o] =
        // its base, obox[SHARD_MAX + o] = slots used); a run that does not fit
        // continues in a fresh chunk (one atomic per OBOX_CHUNK records, no holes)
        unsigned long long b1 = 0, b2 = 0;
        int room = 0;
        if (ocnt > 0) {
          const unsigned long long b = obox[lane], used = obox[SHARD_MAX + lane];
          room = b == ~0ull ? 0 : (int)(OBOX_CHUNK - used);
          b1 = b + used;
          if (ocnt > room) {
            b2 = atomicAdd(&box.out_count[lane], (unsigned long long)OBOX_CHUNK);
            obox[lane] = b2;
            obox[SHARD_MAX + lane] = (unsigned long long)(ocnt - room);
          } else {
            obox[SHARD_MAX + lane] = used + (unsigned long long)ocnt;
          }
        }
        const int src = rem ? powner : 0;
        b1 = shfl_u64(b1, src);
        b2 = shfl_u64(b2, src);
        room = __shfl(room, src);
        const int r = __popcll(mym & lanes_below);
        const unsigned long long slot = r < room ? b1 + r : b2 + (r - room);
        const unsigned long long ref = outbox_ref(s0 + (rinfo >> 16), rinfo & 0xffffu);
        if (rem && slot < box.cap) outbox_put(box, powner, slot, pf, ref);
        // past the region's end (the groups in flight when it filled): the
        // overflow list, sent next round (overflow_put, rtla_kdev.h, spelled
        // out: the call changes the N = 1 SYMMETRY kernel's register allocation)
        const bool ov = rem && slot >= box.cap;
        const unsigned long long om = __ballot(ov);
        if (om) {
          unsigned long long ob = 0;
          if (lane == 0) ob = atomicAdd(box.over_count, (unsigned long long)__popcll(om));
          ob = shfl0_u64(ob);
          if (ov) {
            const unsigned long long k = ob + __popcll(om & lanes_below);
            if (k < box.over_cap) {
              box.over_fp[2 * k] = pf.a;
              box.over_fp[2 * k + 1] = pf.b;
              box.over_ref[k] = ref;
            } else {
              set_flag(ctr, FLAG_OUTBOX_FULL);
            }
          }
        }
      }
    }
    const unsigned long long m = __ballot(isnew);
    if (m && (xflags & XF_DEDUP_ONLY)) {  // synthetic microbench: count, keep no row
      dedup_new += __popcll(m);
    } else if (m) {
      if (isnew) newl[(tail + __popcll(m & lanes_below)) & (NEWCAP - 1)] = (uint16_t)((ninfo >> 16) << 8 | (ninfo & 255u));
      tail += __popcll(m);
      wave_sync();
    }
    pend = false;
  };

  // ---- one chunk: lane t evaluates ring entry done + t (tile row << 8 |
  // instance).  The outcome -- whether and where it probes -- is kept for
  // issue_probe(), which runs after the previous chunk's probes resolved.
  bool nprobe = false;
  unsigned long long nidx = 0;
  FP ncf{0, 0};
  int nowner = me;
  uint32_t ninfo_new = 0;
  auto eval_chunk = [&](int done, int cnt) {
    const bool active = lane < cnt;
    const int e = active ? ring[(done + lane) & (RING - 1)] : 0;
    const int sl = e >> 8, inst = e & 255;
    const uint32_t* prow = rows + sl * W;
    const FP qfp = pfpl[sl];
    DeltaFpT<NS> d;
    d.enabled = 0;
    if (!(xflags & XF_NO_DELTA)) chunk_delta(active, prow, inst, d);
    const bool en = enabled_ok(&ctr->flags, d.enabled != 0, d.err);
    my_gen += en ? 1u : 0u;
    bool kq = false;
    nprobe = false;
    nidx = 0;
    ncf = FP{0, 0};
    nowner = me;
    ninfo_new = (uint32_t)sl << 16 | (uint32_t)inst;
    if (en && (xflags & XF_ALL_SUCCESSORS)) {
      nprobe = true;  // "probe" = output it: issue_probe skips the load, resolve takes it as new
    } else if (en && d.in_model) {
      const FP cfp = (xflags & XF_NO_HASH) ? FP{qfp.a + d.rec[0] + (uint64_t)d.fmsg.a, qfp.b + d.rec[1]}
                                           : fp_add(qfp, delta_fp<NS>(L, prow, d));
      const FP qfp0 = row_fp(prow);
      if (cfp.a != qfp0.a || cfp.b != qfp0.b) {  // successor == parent: already in the set
        if constexpr (SYM) {
          kq = true;  // its seen-set key is the orbit key: queued for key_chunk
        } else {
          const FP key = cfp;  // seen-set key: the fingerprint
          nprobe = !(xflags & XF_NO_PROBE);
          ncf = key;
          nowner = MULTI ? fp_owner(key, box.nshard) : me;
          nidx = (MULTI && nowner != me) ? home_slot(key, box.slog2) : key.a >> (64 - tlog2);
        }
      }
    }
    if constexpr (SYM) {
      const unsigned long long km = __ballot(kq);
      if (kq) kring[(kpos + __popcll(km & lanes_below)) & (RING - 1)] = (uint16_t)(sl << 8 | inst);
      kpos += __popcll(km);
    }
    cover_add(cov, en, inst, d.sub);  // generated coverage
    // out-of-model successors: checked, never stored (not in the
    // synthetic microbench, whose random states are no model's)
    int bad = 0;
    if (en && !d.in_model && !(xflags & (XF_DEDUP_ONLY | XF_ALL_SUCCESSORS)))
      bad = check_invariants_v<NS>(L, prow, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]);
    if (claim_violation(ctr, bad, lane)) record_violation(ctr, cur_base + s0 + sl, inst, 0, ~0ull);
  };
  // SYMMETRY: orbit keys, one successor per lane: the ccount continuations
  // first, then kring[kd, kd + kc) -- the full Delta (the probe pass only
  // folded it into a hash), the signatures, and ONE permutation image per
  // pass (`last`: all that are left); a successor with more images left
  // continues in the next key chunk, the others' keys go through the probe
  // pipeline.  Images computed one per pass keep the wave from waiting for
  // its slowest lane: configs[3]'s successors compare 1.15 images on average
  // but the slowest lane of a 64-successor chunk 2.31 (level-15 successors,
  // tools/symstat.cpp; profiles/r04_v4/symstat.txt).
  // Kept apart from the evaluation pass so that neither holds the other's
  // registers.  (Spreading one successor's images over several lanes was
  // built and measured: 2.1-2.4x slower, the recomputed Deltas and the LDS
  // min-reduction cost more than the divergence they remove.)
  auto key_chunk = [&](int kd, int kc, bool last) {
    const int cn = ccount;
    const bool cont = lane < cn;
    const bool active = lane < cn + kc;
    int e = 0, k = 0;
    if (cont) {
      const uint32_t ce = cent[lane];
      e = (int)(ce & 0xffffu);
      k = (int)(ce >> 16);
    } else if (active) {
      e = kring[(kd + lane - cn) & (RING - 1)];
    }
    const int sl = e >> 8, inst = e & 255;
    const uint32_t* prow = rows + sl * W;
    nprobe = false;
    ninfo_new = (uint32_t)sl << 16 | (uint32_t)inst;
    int next = -1;
    FP best{~0ull, ~0ull};
    if (active) {
      const KeyStep ks = key_one<NS, LC, GROUP>(Lrt, prow, sigl + sl, inst, k, last,
                                                cont ? cbest[lane] : FP{~0ull, ~0ull}, afpl[sl]);
      next = ks.next < 0 ? -1 : ks.next;
      best = ks.f;
      if (ks.next == -1) {
        const FP key = ks.f;
        nprobe = !(xflags & XF_NO_PROBE);
        ncf = key;
        nowner = MULTI ? fp_owner(key, box.nshard) : me;
        nidx = (MULTI && nowner != me) ? home_slot(key, box.slog2) : key.a >> (64 - tlog2);
      }
    }
    const unsigned long long cm = __ballot(next >= 0);
    wave_sync();  // (every lane has read its continuation)
    if (next >= 0) {
      const int c = __popcll(cm & lanes_below);
      cent[c] = (uint32_t)e | (uint32_t)next << 16;
      cbest[c] = best;
    }
    ccount = __popcll(cm);
    wave_sync();
  };
  auto issue_probe = [&]() {
    asm volatile("" ::: "memory");
    issue_cas();
    if (nprobe) {
      my_probe++;
      pend = true;
      pf = ncf;
      pinfo = ninfo_new;
      unsigned long long* slotp = &((MULTI && nowner != me) ? sent : table)[nidx];
      // load first: most successors are already in the set, and a plain
      // load is cheaper than an atomic at the memory side; the CAS is
      // only issued (at resolve time) when the home slot reads empty
      if (MULTI && nowner != me && !box.slog2)
        pold = 0ull;  // no sent cache: every remote successor is queued for its owner
      else if (!(xflags & XF_ALL_SUCCESSORS))
        pold = ((xflags & XF_CAS_ONLY) && !(MULTI && nowner != me))
                   ? atomicCAS(slotp, 0ull, ncf.b | 1ull)
                   : __hip_atomic_load(slotp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    nprobe = false;
  };
  // Every probe in flight resolved: the last loads, then the CAS they set up.
  auto drain = [&]() {
    resolve();
    if (async_cas) {
      issue_cas();
      resolve();
    }
  };
  // Append the pairs of instance q (bit q of this window's wave-wide mask)
  // to the ring, Receive grouped by message type (one handler of
  // raft.tla:421-436 per run).
  auto append_instance = [&](int& pos, unsigned long long mask, int wb, int q, const uint32_t* prow_mine, int f) {
    const bool mine = (mask >> q) & 1ull;
    if (recv_group && f == F_RECEIVE) {
      const uint32_t ty = mine ? slot_type(L, prow_mine, wb + q - L.fam[F_RECEIVE]) : 0u;
#pragma unroll
      for (uint32_t t = 0; t < 4; t++) {
        const bool b = mine && ty == t;
        const unsigned long long m = __ballot(b);
        if (b) ring[(pos + __popcll(m & lanes_below)) & (RING - 1)] = (uint16_t)(lane << 8 | (wb + q));
        pos += __popcll(m);
      }
    } else {
      const unsigned long long m = __ballot(mine);
      if (mine) ring[(pos + __popcll(m & lanes_below)) & (RING - 1)] = (uint16_t)(lane << 8 | (wb + q));
      pos += __popcll(m);
    }
  };

  // Groups are handed out by a device-wide counter (one atomic per group,
  // the next one requested while the current group is processed): a wave
  // that became resident late, or drew heavy groups, simply takes fewer --
  // no static partition, no tail.  (The occupancy API can over-report the
  // resident blocks by one per CU; a static stride would then serialise 1/k
  // of the work behind the rest.)
  // MULTI: a wave takes its next group at the end of the current one, and
  // only while no owner region of the outbox has reached box.stop_at; the
  // groups taken are always a prefix [0, group_next) of the range, so the
  // driver continues the level from there in the next exchange round.  At
  // most two groups per wave run after a region fills (the overflow list's
  // capacity covers them).
  auto take_group = [&]() -> unsigned long long {
    const bool full = MULTI && lane < box.nshard && lane != me &&
                      __hip_atomic_load(&box.out_count[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= box.stop_at;
    unsigned long long g = ~0ull;
    if (!__ballot(full) && lane == 0) g = atomicAdd(&ctr->group_next, 1ull);
    return g;
  };
  if (MULTI && blockIdx.x == 0 && lane == 0 && wave == 0) ctr->group_size = GROUP;
  unsigned long long gnext = 0;
  if (MULTI) gnext = take_group();
  else if (lane == 0) gnext = atomicAdd(&ctr->group_next, 1ull);
  const unsigned long long ngroups = (s_end - s_begin + GROUP - 1) / GROUP;
  [[maybe_unused]] uint32_t pfa_c = 0, pfb_c = 0;  // the group end's touches of the next tile's lines (below), carried to the next group
  for (unsigned long long gi = shfl0_u64(gnext); gi < ngroups; gi = shfl0_u64(gnext)) {
    if (!MULTI && lane == 0) gnext = atomicAdd(&ctr->group_next, 1ull);
    s0 = s_begin + gi * GROUP;
    const int nvalid = (int)min<unsigned long long>((unsigned long long)GROUP, s_end - s0);
    {  // s0 and cur.start are multiples of GROUP: the group's rows are contiguous in the arena
      const uint32_t* src = ring_row(cur, s0, W);
      const int nw = nvalid * W;
      // 16-byte aligned: s0 * W * 4 is a multiple of 128 * W, and the row tile's LDS offset of 16
      // By LDS-DMA: every piece of the tile is requested before the wave waits for any, with no staging
      // registers (a register-staged copy came out as one load, one wait, one LDS write at a time in
      // these kernels: rtla_kdev.h).  The previous group's row build may still have LDS reads of the
      // tile in flight, and a DMA write is not ordered behind them: they are waited for first (the
      // build has consumed them all by now).  The tile is read only after the DMA's own wait.
      // (Every instantiation: configs[1] 150.7-153.3 -> 140.6-142.5 ms, the narrow-row exhaust model
      // 1123-1125 -> 1101-1103 ms; profiles/r12_tile/tile_ab.txt)
      lds_reads_done();
      if (RTLA_IDX_OK(ctr, ring_idx(cur, s0) + nvalid, cur.cap + 1)) copy_words_lds_dma(rows, src, nw, lane);
      dma_wait();
    }
    if constexpr (!narrow)  // (the previous group end's line touches: returned before this tile did)
      asm volatile("" ::"v"(pfa_c), "v"(pfb_c));
    wave_sync();
    STAMP(8);  // row tile load (and the wait for the work-queue atomic issued before it)
    // the next group's number (its atomic returned before the tile copy's wait; MULTI: taken at the group's end)
    unsigned long long gnn = MULTI ? 0ull : shfl0_u64(gnext);
    const bool valid = lane < nvalid;
    const uint32_t* prow_mine = rows + (lane & (GROUP - 1)) * W;
    int nmsg = 0;
    if (valid) {
      pfpl[lane] = fp_add(row_fp(prow_mine), alllogs_delta<NS>(L, prow_mine, pall_mine));
      if (SYM) afpl[lane] = alllogs_fp(L, pall_mine);
      nmsg = row_nmsg(L, prow_mine);
      if constexpr (SYM) {
        uint32_t loc[NS], ms[NS], mr[NS];
        sym_sig_parts<NS>(L, [&](int i, uint32_t* out) { load_rec<NS>(L, prow_mine, i, out); }, nmsg,
                          [&](int q) { return slot_raw(L, prow_mine, q); }, loc, ms, mr);
#pragma unroll
        for (int j = 0; j < NS; j++) {
          sigl[j * GROUP + lane] = loc[j];
          sigl[(NS + j) * GROUP + lane] = ms[j];
          sigl[(2 * NS + j) * GROUP + lane] = mr[j];
        }
      }
    }
    wave_sync();
    STAMP(0);  // per-state setup
    // With at most one copy of a message allowed (max copies 1), every
    // DuplicateMessage successor (raft.tla:443-445) is out of the model: its
    // one message's count becomes 2 (specs/MC.tla).  It differs from its
    // parent in the bag alone, so the invariants -- which read servers and
    // elections only -- hold on it as on the parent (every expanded state
    // passed them, or the run stopped at its level).  Such successors are
    // counted (generated, per-action coverage: one per message of the bag),
    // not evaluated -- 1/6 of configs[1]'s successors.  The successor walks
    // (XF_ALL_SUCCESSORS) still list them.
    // (kept per lane and reduced once at the end -- configs[1] 180.3 -> 178.5
    // ms; the SYMMETRY kernel keeps the per-group reduction: 292.1 -> 285.8)
    if (dup_counted) {
      if constexpr (SYM) {
        if (valid) my_gen += (unsigned)nmsg;
        if (!(xflags & XF_NO_COVER)) {
          int nd = valid ? nmsg : 0;
          for (int off = 32; off > 0; off >>= 1) nd += __shfl_down(nd, off);
          if (lane == 0 && nd) atomicAdd(&cov[F_DUPLICATE], (unsigned)nd);
        }
      } else if (valid) {
        my_dup += (unsigned)nmsg;
      }
    }
    for (int wb = 0; wb < ((xflags & XF_NO_CHUNKS) ? 0 : ninst); wb += 64) {
      const unsigned long long mask = valid ? cand_mask<NS>(L, prow_mine, nmsg, wb, !dup_counted) : 0ull;
      unsigned long long todo = wave_or_u64(mask);
      int pos = 0, done = 0;
      while (todo || pos > done) {
        // Append the pairs of the next instance(s) until a chunk is ready (cut
        // at a family boundary once family_cut pairs are queued).
        int cfam = -1;
        while (todo && pos - done < 64) {
          const int q = __builtin_ctzll(todo);
          const int f = inst_family(L, wb + q);
          if (f != cfam && pos - done >= family_cut) break;
          cfam = f;
          todo &= todo - 1;
          append_instance(pos, mask, wb, q, prow_mine, f);
        }
        const int cnt = min(64, pos - done);
        wave_sync();
        STAMP(1);  // pair ring
        eval_chunk(done, cnt);
        STAMP(2);  // successor deltas, fingerprints, coverage, out-of-model invariants
        if (!SYM || (xflags & XF_ALL_SUCCESSORS)) {
          resolve();  // the previous chunk's probes, after this chunk's arithmetic
          STAMP(3);
          issue_probe();
          STAMP(4);  // probe issue
        } else {
          // 64 orbit keys to compute (continuations first): key them (they
          // feed the probe pipeline) until fewer than 64 are queued (the key
          // ring holds RING = 128; an evaluation chunk adds at most 64)
          while (kpos - kdone + ccount >= 64) {
            const int kc = min(kpos - kdone, 64 - ccount);
            key_chunk(kdone, kc, kc == 0);
            kdone += kc;
            STAMP(7);  // SYMMETRY: orbit keys
            resolve();
            STAMP(3);
            issue_probe();
            STAMP(4);  // probe issue
          }
        }
        if (tail - head > NEWFLUSH) {  // rare (early levels): drain the probes, build the rows so far
          drain();
          build_all();
          STAMP(5);
        }
        done += cnt;
      }
    }
    // Group end: the last probes and every pending row (their parents are
    // this group's rows, which the next group overwrites).
    // Touch every 128-byte line of the next group's rows now, so that its
    // tile load after this drain hits the caches.  Relaxed atomic loads: the
    // compiler issues them here (it does not sink an atomic) and tracks
    // their destination registers like any load (its vmcnt waits count
    // them); the values are consumed only after the next group's tile load,
    // so nothing waits for them before.  (an asm-issued load's
    // register was invisible to the compiler.)
    [[maybe_unused]] uint32_t pfa = 0, pfb = 0;  // (the narrow-row kernels': consumed at this group's end)
    pfa_c = pfb_c = 0;
    if (MULTI) {
      gnext = take_group();
      gnn = shfl0_u64(gnext);
    }
    while (SYM && kpos - kdone + ccount > 0) {  // the group's last orbit keys (they key this group's rows)
      const int kc = min(kpos - kdone, 64 - ccount);
      key_chunk(kdone, kc, kc == 0 || kpos - kdone + ccount <= 64);  // (the last chunk: every image left)
      kdone += kc;
      STAMP(7);
      resolve();
      issue_probe();
    }
    if (gnn < ngroups) {
      const unsigned long long sn = s_begin + gnn * GROUP;
      const int lines = ((int)min<unsigned long long>((unsigned long long)GROUP, s_end - sn) * W + 31) / 32;
      const uint32_t* pa = ring_row(cur, sn, W) + 32 * min(lane, lines - 1);
      const uint32_t* pb = ring_row(cur, sn, W) + 32 * min(lane + 64, lines - 1);
      if constexpr (narrow) {
        pfa = __hip_atomic_load(pa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pfb = __hip_atomic_load(pb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        pfa_c = __hip_atomic_load(pa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pfb_c = __hip_atomic_load(pb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    drain();
    if constexpr (!SYM) STAMP(7);  // (non-symmetric builds: slot 7 = the group-end probe drain alone)
    build_all();
    // No wait for the row and parent-record stores here (nothing reads them
    // back in this launch; vmcnt counts stores too, so a wait for the two
    // touches above would drain them all): the next group's tile load is
    // issued behind them, and its own wait -- which it needs anyway -- is the
    // first to cover them.  The tile may be overwritten: the row build read
    // it from LDS into registers before storing; a register-staged tile copy
    // writes LDS behind those reads (LDS operations of a wave complete in
    // order), the LDS-DMA one waits for them itself (lds_reads_done at the
    // head of the loop).  (The narrow-row kernels keep the wait and
    // consume the touches here: carried over the loop they cost the
    // 128-VGPR kernel 20-90 ms per exhaust-model run.)
    if constexpr (narrow) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("" ::"v"(pfa), "v"(pfb));
    }
    wave_sync();
    STAMP(6);  // group-end drain
  }
  if (MULTI) {
    for (int o = 0; o < box.nshard; o++) {
      const unsigned long long b = obox[o], used = obox[SHARD_MAX + o];
      if (b != ~0ull) outbox_holes(box, o, b + used, b + OBOX_CHUNK, lane);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    my_gen += __shfl_down(my_gen, off);
    my_probe += __shfl_down(my_probe, off);
    my_dup += __shfl_down(my_dup, off);
  }
  my_gen += my_dup;
  if (lane == 0 && my_dup && !(xflags & XF_NO_COVER)) atomicAdd(&cov[F_DUPLICATE], my_dup);
  if (lane == 0 && my_gen) atomicAdd(&ctr->generated, (unsigned long long)my_gen);
  if (lane == 0 && my_probe) atomicAdd(&ctr->probes, (unsigned long long)my_probe);
  if (lane == 0 && dedup_new) atomicAdd(&ctr->next_count, dedup_new);
#ifdef RTLA_COUNT_CAS
  for (int off = 32; off > 0; off >>= 1) my_cas += __shfl_down(my_cas, off);
  if (lane == 0 && my_cas) atomicAdd(&ctr->cas, (unsigned long long)my_cas);
#endif
  STAMP(7);  // (kernel end: negligible)
  RTLA_STAMP_FLUSH(ctr, lane)
  cover_flush(cov, 2 * COVER_CODES, ctr->cover);
}

namespace rtla {

// States per wave-group of k_expand_compact: 64, or 32 when 64 rows would
// make the per-wave LDS tile so large that fewer than ~11 waves fit a CU.
#ifndef RTLA_GROUP64_LDS
#define RTLA_GROUP64_LDS (16 * 1024)
#endif
// SYMMETRY: always 32 (one instantiation per N; the orbit-key arithmetic,
// not the tile, bounds that kernel).
constexpr int compact_group(const Layout& L) {
  if (L.sym) return 32;
  return compact_lds_words(L.W, L.all_words, 64, false, true) * sizeof(uint32_t) <= RTLA_GROUP64_LDS ? 64 : 32;
}
// The compiled-in configurations may also run 16-state groups: wide rows
// (configs[2]: 516 B, configs[3]: 628 B) would otherwise leave the 32-row
// tile, not the registers, bounding the waves per CU (8 and 7 instead of
// 12 and 8; bench's occupancy sweep: throughput grows with resident waves).
#ifndef RTLA_GROUP32_LDS
#define RTLA_GROUP32_LDS (19 * 1024)
#endif
#ifndef RTLA_SYM_GROUP
#define RTLA_SYM_GROUP 16
#endif
constexpr int spec_group(const Layout& L) {
  if (L.sym) return RTLA_SYM_GROUP;  // configs[3]: 16 waves/CU at 128 VGPRs need the smaller tile (311.5 vs 322 ms)
  const int g = compact_group(L);
  return g == 32 && compact_lds_words(L.W, L.all_words, 32, L.sym, true) * sizeof(uint32_t) > RTLA_GROUP32_LDS ? 16 : g;
}

template <int NS, int GROUP, Layout LC, bool SYM = false>
static hipError_t launch_compact(const LevelArgs& a) {
  const Layout& L = a.L;
  const bool multi = a.box.nshard > 1;
  const int xflags = a.xflags;
  const int wpb = (xflags & XF_BLOCK4) ? expand_compact_wpb(L) : 1;  // one-wave workgroups by default
  const uint64_t s_begin = a.s_begin, s_end = a.s_end;
  DevCounters* ctr = a.ctr;
  hipStream_t st = a.st;
  auto kfn = multi ? k_expand_compact<NS, true, GROUP, LC, SYM> : k_expand_compact<NS, false, GROUP, LC, SYM>;
  const uint64_t groups = (s_end - s_begin + GROUP - 1) / GROUP;
  uint64_t blocks = std::min<uint64_t>((groups + wpb - 1) / wpb, 1u << 20);
  const size_t lds = (size_t)wpb * compact_lds_words(L.W, L.all_words, GROUP, SYM, multi) * sizeof(uint32_t);
  if (!(xflags & XF_NO_PERSIST) || a.query) {  // persistent waves: exactly the resident capacity, looping over groups
    static int per_cu[2][2];  // per instantiation: [multi][one-wave blocks]
    int& pc = per_cu[multi][wpb == 1];
    if (!pc) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, kfn, 64 * wpb, lds) != hipSuccess || pc < 1)
        pc = 16 / wpb;
      if (const char* e = getenv("RTLA_BLOCKS_PER_CU"))  // occupancy experiments
        if (atoi(e) > 0) pc = std::min(pc, atoi(e));
    }
    blocks = std::min<uint64_t>(blocks, (uint64_t)device_cus() * pc);
    if (a.query) {  // level_kernel_shape: the waves resident at once (any launch mode) and the group size
      a.query[0] = device_cus() * pc * wpb;
      a.query[1] = GROUP;
      return hipSuccess;
    }
  }
  {
    hipError_t e = hipMemsetAsync(&ctr->group_next, 0, sizeof(ctr->group_next), st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)blocks), dim3(64 * wpb), lds, st, L, a.cur, (unsigned long long)s_begin,
                     (unsigned long long)s_end, (unsigned long long)a.cur_base, a.out.next,
                     (unsigned long long*)a.out.parents, (unsigned long long)a.out.next_base,
                     (unsigned long long)a.out.next_cap, (unsigned long long*)a.table, (unsigned long long*)a.sent, a.tlog2, ctr, a.box, xflags);
  return hipGetLastError();
}

}  // namespace rtla
