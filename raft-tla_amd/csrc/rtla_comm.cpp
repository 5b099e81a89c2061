// rtla_comm.cpp -- how bytes get from one shard to another: the collectives
// between ranks (RCCL, or the shared-memory transport) and the transfers of
// an exchange round (Exchange).  The only unit that knows which transport a
// context runs on; the deployments are listed in rtla_host.cpp.
#include <fcntl.h>
#include <rccl/rccl.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>

#include "rtla_ctx.h"

// Host shared-memory transport for world > 1 (RTLA_TRANSPORT=shm): the same
// collectives as the RCCL path, staged through a POSIX shared-memory segment
// named after the communicator id.  It lets N processes on ONE GPU run the
// multi-rank protocol -- RCCL refuses two ranks on one device -- so the
// world > 1 control flow (count gathers, all-to-all-v, answer routing,
// reductions, trace broadcasts, recovery checks) is tested on single-GPU
// boxes.  Not a performance path: every operation synchronises the stream.
struct ShmComm {
  struct Header {
    std::atomic<uint32_t> arrive, gen;
    std::atomic<uint32_t> abort;  // a rank failed inside a collective: every wait ends (RTLA_E_COMM)
  };
  Header* hdr = nullptr;
  uint8_t* data = nullptr;   // world x world slots of `slot` bytes: [src][dst]
  size_t slot = 0, size = 0;
  uint8_t* slot_at(int src, int dst, int world) const { return data + ((size_t)src * world + dst) * slot; }
};

struct Comm {
  ncclComm_t nccl = nullptr;
  ShmComm* shm = nullptr;   // RTLA_TRANSPORT=shm instead of RCCL
  bool rccl_local = false;  // world 1, S shards, RTLA_TRANSPORT=rccl: the exchange goes through `nccl` (1 rank)
};

static int shm_barrier(rtla_ctx* x) {
  ShmComm::Header* h = x->comm->shm->hdr;
  if (h->abort.load(std::memory_order_acquire)) return RTLA_E_COMM;
  const uint32_t g = h->gen.load(std::memory_order_acquire);
  if (h->arrive.fetch_add(1, std::memory_order_acq_rel) == (uint32_t)x->world - 1) {
    h->arrive.store(0, std::memory_order_relaxed);
    h->gen.fetch_add(1, std::memory_order_acq_rel);
    return RTLA_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  while (h->gen.load(std::memory_order_acquire) == g) {
    if (h->abort.load(std::memory_order_acquire)) {
      fprintf(stderr, "rtla: shm transport: another rank failed inside a collective\n");
      return RTLA_E_COMM;
    }
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(600)) {
      fprintf(stderr, "rtla: shm transport: the other ranks did not arrive\n");
      return RTLA_E_COMM;
    }
    sched_yield();
  }
  return RTLA_OK;
}

static int shm_open_comm(rtla_ctx* x, const void* comm_id) {
  const uint8_t* id = static_cast<const uint8_t*>(comm_id);
  uint64_t h = 1469598103934665603ull;  // FNV-1a of the 128-byte id
  for (int i = 0; i < 128; i++) h = (h ^ id[i]) * 1099511628211ull;
  char name[64];
  snprintf(name, sizeof name, "/rtla_%016llx", (unsigned long long)h);
  const char* e = getenv("RTLA_SHM_SLOT_MB");
  const size_t slot = (size_t)(e && atoi(e) > 0 ? atoi(e) : 64) << 20;
  const size_t size = 4096 + (size_t)x->world * x->world * slot;
  const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);
  if (fd < 0) return RTLA_E_COMM;
  if (ftruncate(fd, (off_t)size) != 0) {
    close(fd);
    return RTLA_E_COMM;
  }
  void* p = mmap(nullptr, size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (p == MAP_FAILED) return RTLA_E_COMM;
  ShmComm* c = x->comm->shm = new ShmComm();
  c->hdr = static_cast<ShmComm::Header*>(p);
  c->data = static_cast<uint8_t*>(p) + 4096;
  c->slot = slot;
  c->size = size;
  const int rc = shm_barrier(x);  // every rank has the segment mapped: the name can go
  if (x->rank == 0) shm_unlink(name);
  return rc;
}

static int shm_fail(const ShmComm& c, int rc) {  // a local failure inside a collective: the peers' waits end too
  c.hdr->abort.store(1, std::memory_order_release);
  return rc;
}

static int shm_too_big(size_t bytes, const ShmComm& c) {
  if (bytes <= c.slot) return RTLA_OK;
  fprintf(stderr, "rtla: shm transport: %zu-byte message exceeds the %zu-byte slot (RTLA_SHM_SLOT_MB)\n", bytes, c.slot);
  return shm_fail(c, RTLA_E_COMM);
}

// A HIP call inside an shm collective: on failure mark the abort before returning.
#define SHMCHK(c, x) HIPCHK_RET(x, shm_fail((c), RTLA_E_HIP))

static int nccl_rc(ncclResult_t r, int line) {  // an RCCL result as a status; a failure is reported
  if (r == ncclSuccess) return RTLA_OK;
  fprintf(stderr, "rtla: RCCL error %s at %s:%d\n", ncclGetErrorString(r), __FILE__, line);
  return RTLA_E_COMM;
}

// In place: sum (op 0) or max (op 1) of n u64 over all ranks.
static int comm_allreduce(rtla_ctx* x, uint64_t* buf, int n, int op) {
  if (!x->comm->shm)
    return nccl_rc(ncclAllReduce(buf, buf, n, ncclUint64, op ? ncclMax : ncclSum, x->comm->nccl, x->stream), __LINE__);
  const ShmComm& c = *x->comm->shm;
  if (int rc = shm_too_big(8 * (size_t)n, c)) return rc;
  SHMCHK(c, hipMemcpyAsync(c.slot_at(x->rank, 0, x->world), buf, 8 * n, hipMemcpyDeviceToHost, x->stream));
  SHMCHK(c, hipStreamSynchronize(x->stream));
  if (int rc = shm_barrier(x)) return rc;
  std::vector<uint64_t> acc(n, 0);
  for (int r = 0; r < x->world; r++) {
    const uint64_t* v = reinterpret_cast<const uint64_t*>(c.slot_at(r, 0, x->world));
    for (int i = 0; i < n; i++) acc[i] = op ? std::max(acc[i], v[i]) : acc[i] + v[i];
  }
  if (int rc = shm_barrier(x)) return rc;
  SHMCHK(c, hipMemcpyAsync(buf, acc.data(), 8 * n, hipMemcpyHostToDevice, x->stream));
  SHMCHK(c, hipStreamSynchronize(x->stream));
  return RTLA_OK;
}

// recv[r * n + i] = send[i] of rank r.
static int comm_allgather(rtla_ctx* x, const uint64_t* send, uint64_t* recv, int n) {
  if (!x->comm->shm) return nccl_rc(ncclAllGather(send, recv, n, ncclUint64, x->comm->nccl, x->stream), __LINE__);
  const ShmComm& c = *x->comm->shm;
  if (int rc = shm_too_big(8 * (size_t)n, c)) return rc;
  SHMCHK(c, hipMemcpyAsync(c.slot_at(x->rank, 0, x->world), send, 8 * n, hipMemcpyDeviceToHost, x->stream));
  SHMCHK(c, hipStreamSynchronize(x->stream));
  if (int rc = shm_barrier(x)) return rc;
  for (int r = 0; r < x->world; r++)
    SHMCHK(c, hipMemcpyAsync(recv + (size_t)r * n, c.slot_at(r, 0, x->world), 8 * n, hipMemcpyHostToDevice, x->stream));
  SHMCHK(c, hipStreamSynchronize(x->stream));
  return shm_barrier(x);
}

static int comm_bcast(rtla_ctx* x, uint64_t* buf, int n, int root) {
  if (!x->comm->shm) return nccl_rc(ncclBroadcast(buf, buf, n, ncclUint64, root, x->comm->nccl, x->stream), __LINE__);
  const ShmComm& c = *x->comm->shm;
  if (int rc = shm_too_big(8 * (size_t)n, c)) return rc;
  if (x->rank == root) {
    SHMCHK(c, hipMemcpyAsync(c.slot_at(root, 0, x->world), buf, 8 * n, hipMemcpyDeviceToHost, x->stream));
    SHMCHK(c, hipStreamSynchronize(x->stream));
  }
  if (int rc = shm_barrier(x)) return rc;
  if (x->rank != root) {
    SHMCHK(c, hipMemcpyAsync(buf, c.slot_at(root, 0, x->world), 8 * n, hipMemcpyHostToDevice, x->stream));
    SHMCHK(c, hipStreamSynchronize(x->stream));
  }
  return shm_barrier(x);
}

// One all-to-all-v round: point-to-point messages (at most one send and one
// receive per peer), all in flight together (one RCCL group).  The group is
// always closed, also when a send or receive could not be posted.
static int comm_exchange(rtla_ctx* x, const std::vector<Msg>& sends, const std::vector<Msg>& recvs) {
  if (!x->comm->shm) {
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess) return nccl_rc(r, __LINE__);
    for (const Msg& m : sends)
      if (r == ncclSuccess) r = ncclSend(m.ptr, m.bytes, ncclUint8, m.peer, x->comm->nccl, x->stream);
    for (const Msg& m : recvs)
      if (r == ncclSuccess) r = ncclRecv(m.ptr, m.bytes, ncclUint8, m.peer, x->comm->nccl, x->stream);
    const ncclResult_t r2 = ncclGroupEnd();
    return nccl_rc(r == ncclSuccess ? r2 : r, __LINE__);
  }
  const ShmComm& c = *x->comm->shm;
  for (const Msg& m : sends) {
    if (int rc = shm_too_big(m.bytes, c)) return rc;
    SHMCHK(c, hipMemcpyAsync(c.slot_at(x->rank, m.peer, x->world), m.ptr, m.bytes, hipMemcpyDeviceToHost, x->stream));
  }
  SHMCHK(c, hipStreamSynchronize(x->stream));
  if (int rc = shm_barrier(x)) return rc;
  for (const Msg& m : recvs) {
    if (int rc = shm_too_big(m.bytes, c)) return rc;
    SHMCHK(c, hipMemcpyAsync(m.ptr, c.slot_at(m.peer, x->rank, x->world), m.bytes, hipMemcpyHostToDevice, x->stream));
  }
  SHMCHK(c, hipStreamSynchronize(x->stream));
  return shm_barrier(x);
}

// The four cases of a transfer.  Both shards local: a device copy, issued at
// once; or (rccl_local) a send and a receive to rank 0 -- this process --
// pushed TOGETHER: the one-rank group pairs the i-th send with the i-th
// receive, so the two lists must stay in step.  One side local: its half of
// the message to the rank that holds the other shard (rank == shard id).
int Exchange::move(int src_shard, const void* src, int dst_shard, void* dst, size_t bytes) {
  if (src && dst && !x->comm->rccl_local) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, x->stream));
    return RTLA_OK;
  }
  const bool both = src && dst;
  if (src) sends.push_back({const_cast<void*>(src), bytes, both ? 0 : dst_shard});
  if (dst) recvs.push_back({dst, bytes, both ? 0 : src_shard});
  return RTLA_OK;
}

// world > 1 exchanges even with nothing queued: the peers wait in it (shm barriers).
int Exchange::flush() {
  return x->world > 1 || !sends.empty() ? comm_exchange(x, sends, recvs) : RTLA_OK;
}

int allreduce2_u64(rtla_ctx* x, uint64_t* sum, int n1, uint64_t* mx, int n2) {
  if (x->world == 1 && !x->comm->rccl_local) return RTLA_OK;
  if (n1 > RED_MAX_AT || RED_MAX_AT + n2 > RED_WORDS) return RTLA_E_ARG;
  HIPCHK(hipMemcpyAsync(x->red, sum, 8 * n1, hipMemcpyHostToDevice, x->stream));
  HIPCHK(hipMemcpyAsync(x->red + RED_MAX_AT, mx, 8 * n2, hipMemcpyHostToDevice, x->stream));
  if (!x->comm->shm) {  // both reductions in one group (closed also when one could not be posted)
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess) return nccl_rc(r, __LINE__);
    r = ncclAllReduce(x->red, x->red, n1, ncclUint64, ncclSum, x->comm->nccl, x->stream);
    if (r == ncclSuccess)
      r = ncclAllReduce(x->red + RED_MAX_AT, x->red + RED_MAX_AT, n2, ncclUint64, ncclMax, x->comm->nccl, x->stream);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess) return nccl_rc(r, __LINE__);
  } else {
    if (int rc = comm_allreduce(x, x->red, n1, 0)) return rc;
    if (int rc = comm_allreduce(x, x->red + RED_MAX_AT, n2, 1)) return rc;
  }
  HIPCHK(hipMemcpyAsync(sum, x->red, 8 * n1, hipMemcpyDeviceToHost, x->stream));
  HIPCHK(hipMemcpyAsync(mx, x->red + RED_MAX_AT, 8 * n2, hipMemcpyDeviceToHost, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  return RTLA_OK;
}

int allreduce_u64(rtla_ctx* x, uint64_t* v, int n, int op) {
  if (x->world == 1 && !x->comm->rccl_local) return RTLA_OK;
  if (n > RED_WORDS) return RTLA_E_ARG;
  HIPCHK(hipMemcpyAsync(x->red, v, 8 * n, hipMemcpyHostToDevice, x->stream));
  if (int rc = comm_allreduce(x, x->red, n, op)) return rc;
  HIPCHK(hipMemcpyAsync(v, x->red, 8 * n, hipMemcpyDeviceToHost, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  return RTLA_OK;
}

int comm_gather_rows(rtla_ctx* x) {
  const int G = x->nshard, RW = G + 2;
  x->h_rows.assign((size_t)G * RW, 0);
  if (x->world > 1) {
    Shard& s = x->sh[0];
    if (int rc = comm_allgather(x, s.out_count, s.all_count, RW)) return rc;
    HIPCHK(hipMemcpyAsync(x->h_rows.data(), s.all_count, 8 * G * RW, hipMemcpyDeviceToHost, x->stream));
  } else {
    for (auto& s : x->sh) {
      const uint64_t* row = s.out_count;
      if (x->comm->rccl_local) {  // (one rank: all_count[0, RW) = out_count)
        if (int rc = comm_allgather(x, s.out_count, s.all_count, RW)) return rc;
        row = s.all_count;
      }
      HIPCHK(hipMemcpyAsync(x->h_rows.data() + (size_t)s.id * RW, row, 8 * RW, hipMemcpyDeviceToHost, x->stream));
    }
  }
  HIPCHK(hipStreamSynchronize(x->stream));
  return RTLA_OK;
}

int comm_parent_record(rtla_ctx* x, uint64_t shard, uint64_t g, bool& bad, uint64_t* p) {
  if (x->world == 1 && !x->comm->rccl_local) {
    HIPCHK(hipMemcpy(p, x->sh[shard].parents + g, 8, hipMemcpyDeviceToHost));
  } else if (x->world == 1) {  // the record travels through the one-rank communicator too
    HIPCHK(hipMemcpyAsync(x->red, x->sh[shard].parents + g, 8, hipMemcpyDeviceToDevice, x->stream));
    if (int rc = comm_bcast(x, x->red, 1, 0)) return rc;
    HIPCHK(hipMemcpyAsync(p, x->red, 8, hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
  } else {
    // the holder contributes the record, every rank its failure flag
    uint64_t w[2] = {0, 0};
    if ((int)shard == x->rank && !bad && hipMemcpy(&w[0], x->sh[0].parents + g, 8, hipMemcpyDeviceToHost) != hipSuccess)
      bad = true;
    w[1] = bad ? 1 : 0;
    if ((int)shard == x->rank && bad) w[0] = 0;
    if (int rc = allreduce_u64(x, w, 2, 0)) return rc;
    if (w[1]) return bad ? RTLA_E_HIP : RTLA_E_COMM;
    *p = w[0];
  }
  return RTLA_OK;
}

// RCCL prints its version banner on stdout when a communicator is created;
// stdout belongs to the caller (the CLI's TLC-format output, bench.py's JSON
// line), so the banner is sent to stderr.
struct StdoutToStderr {
  int saved = -1;
  StdoutToStderr() {
    fflush(stdout);
    saved = dup(1);
    if (saved >= 0) dup2(2, 1);
  }
  ~StdoutToStderr() {
    fflush(stdout);
    if (saved >= 0) {
      dup2(saved, 1);
      close(saved);
    }
  }
};

static bool transport_is(const char* name) {
  const char* tr = getenv("RTLA_TRANSPORT");
  return tr && !strcmp(tr, name);
}

extern "C" int rtla_comm_id(void* out128) {
  if (!out128) return RTLA_E_ARG;
  if (transport_is("shm")) {  // the id only names the shared-memory segment
    uint64_t v[16];
    const uint64_t t = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
    for (int i = 0; i < 16; i++) v[i] = t * 0x9E3779B97F4A7C15ull + (uint64_t)getpid() * 0xBF58476D1CE4E5B9ull + i;
    memcpy(out128, v, 128);
    return RTLA_OK;
  }
  ncclUniqueId id;
  ncclResult_t r0;
  {
    StdoutToStderr quiet;
    r0 = ncclGetUniqueId(&id);
  }
  if (int rc = nccl_rc(r0, __LINE__)) return rc;
  static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
  memcpy(out128, &id, 128);
  return RTLA_OK;
}

// world > 1: RCCL between the ranks, or the shm transport.  world 1 with
// virtual shards: device copies, or (RTLA_TRANSPORT=rccl) a one-rank communicator.
int comm_open(rtla_ctx* x, const void* comm_id) {
  x->comm = new Comm();
  if (x->world > 1 && transport_is("shm")) return shm_open_comm(x, comm_id);
  x->comm->rccl_local = x->world == 1 && x->nshard > 1 && transport_is("rccl");
  if (x->world == 1 && !x->comm->rccl_local) return RTLA_OK;
  ncclUniqueId id;
  ncclResult_t r0 = ncclSuccess;
  StdoutToStderr quiet;
  if (x->world > 1) memcpy(&id, comm_id, sizeof id);
  else r0 = ncclGetUniqueId(&id);
  if (r0 == ncclSuccess) r0 = ncclCommInitRank(&x->comm->nccl, x->world, id, x->rank);
  return r0 == ncclSuccess ? RTLA_OK : RTLA_E_COMM;
}

void comm_close(rtla_ctx* x) {
  if (!x->comm) return;
  if (x->comm->nccl) ncclCommDestroy(x->comm->nccl);
  if (x->comm->shm) {
    munmap(x->comm->shm->hdr, x->comm->shm->size);
    delete x->comm->shm;
  }
  delete x->comm;
  x->comm = nullptr;
}

const char* comm_name(const rtla_ctx* x) {
  return x->comm->shm ? "shm" : x->comm->nccl ? (x->comm->rccl_local ? "rccl-local" : "rccl") : "device";
}
