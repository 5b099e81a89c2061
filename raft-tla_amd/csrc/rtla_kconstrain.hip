// rtla_kconstrain.hip -- the constraint pass's kernels:
// the keep bitmap of a level and the stable, in-place compaction of the level's
// rows in the arena ring and of their parent records.
//
//   k_constrain_pack    the per-row masks of k_pred_state (rtla_kpred.hip) -> one
//                       u64 per group of 64 rows, the ballot of "every definition
//                       true"; the dropped rows are tallied on the device.
// and per chunk of R rows (R a multiple of 64), enqueued in stream order:
//   k_constrain_scan    one block: the chunk's destination (the running total of
//                       kept rows, which stays on the device) and the exclusive
//                       scan of its keep-word popcounts;
//   k_constrain_gather  a wave per group: the group's rows into LDS by 16-byte
//                       loads, the kept ones closed up there, then stored to the
//                       staging buffer, with their parent records;
//   k_constrain_put     the staging buffer back to ring rows base_c .. and to the
//                       parent records at the same indices.
// The destination of chunk c lies at or below its own source range, so it can
// overlap only source rows of chunks <= c, all of them in staging or already
// moved when k_constrain_put(c) runs: STREAM ORDER IS THE ONLY ORDERING.  No
// kernel waits for another workgroup.  A chunk that keeps every row where it
// lies (ConstrainTotals.move == 0) is left alone by the gather and the copy-back.
//
// Rows are W words, W odd, so a run of rows starts at any word alignment.  The
// staging buffer is written at the word shift of its destination in the ring:
// the copy-back then moves 16 bytes per lane with both sides aligned (the part
// of a chunk past the arena's wrap falls back to words where its shift differs).
#include "rtla_kaudit.h"
#include "rtla_constrain.h"

namespace {

constexpr int CONSTRAIN_WPB = 4;
constexpr int SCAN_THREADS = 1024;

__device__ __forceinline__ unsigned long long low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// The word shift of the chunk's destination: staging row k lies at stage + shift + k * W.
__device__ __forceinline__ int dest_shift(const Ring& cur, unsigned long long base, int W) {
  return (int)((ring_idx(cur, base) * (unsigned long long)W) & 3ull);
}

// n words LDS -> global, the destination at any word alignment: words up to its first 16-byte boundary, 16 bytes
// per lane from there, the last words.
__device__ __forceinline__ void store_words_lds(uint32_t* __restrict__ dst, const uint32_t* src, int n, int lane) {
  int head = (int)((4u - (unsigned)((uintptr_t)dst >> 2 & 3u)) & 3u);
  if (head > n) head = n;
  if (lane < head) dst[lane] = src[lane];
  const int n4 = (n - head) >> 2;
  uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst + head);
  const uint32_t* s = src + head;
  for (int q = lane; q < n4; q += 64) d4[q] = make_uint4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
  for (int t = head + (n4 << 2) + lane; t < n; t += 64) dst[t] = src[t];
}

// n words global -> global by the whole grid: 16 bytes per thread where dst and src share their alignment.
__device__ __forceinline__ void copy_words_grid(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                unsigned long long n) {
  const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long nth = (unsigned long long)gridDim.x * blockDim.x;
  if ((((uintptr_t)dst ^ (uintptr_t)src) & 15u) != 0) {
    for (unsigned long long t = tid; t < n; t += nth) dst[t] = src[t];
    return;
  }
  unsigned long long head = (4u - (unsigned)((uintptr_t)dst >> 2 & 3u)) & 3u;
  if (head > n) head = n;
  if (tid < head) dst[tid] = src[tid];
  const unsigned long long n4 = (n - head) >> 2;
  uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst + head);
  const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src + head);
  unsigned long long q = tid;
  for (; q + 3 * nth < n4; q += 4 * nth) {  // four loads in flight per thread
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = s4[q + j * nth];
#pragma unroll
    for (int j = 0; j < 4; j++) d4[q + j * nth] = v[j];
  }
  for (; q < n4; q += nth) d4[q] = s4[q];
  for (unsigned long long t = head + (n4 << 2) + tid; t < n; t += nth) dst[t] = src[t];
}

}  // namespace

// masks[0, n): the false-definition mask of each row -> keep[g] for every group g of 64 rows (rows past n: 0).
__global__ void __launch_bounds__(256) k_constrain_pack(const int* __restrict__ masks, unsigned long long n,
                                                        unsigned long long* __restrict__ keep, ConstrainTotals* tot) {
  const int lane = threadIdx.x & 63;
  const unsigned long long ngroup = (n + 63) >> 6;
  const unsigned long long wave = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const unsigned long long nwave = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
  unsigned long long dropped = 0;
  for (unsigned long long g = wave; g < ngroup; g += nwave) {
    const unsigned long long i = (g << 6) + lane;
    const bool valid = i < n;
    const bool k = valid && masks[i] == 0;
    const unsigned long long word = __ballot(k);
    dropped += __popcll(__ballot(valid)) - __popcll(word);
    if (lane == 0) keep[g] = word;
  }
  if (lane == 0 && dropped) atomicAdd(&tot->dropped, dropped);
}

// One block.  The chunk's rows are level rows [first, first + rows); keep: its rows / 64 (rounded up) keep words.
// tot->base advances over the previous chunk; offs[g] = kept rows of the chunk before group g.
__global__ void __launch_bounds__(SCAN_THREADS)
k_constrain_scan(const unsigned long long* __restrict__ keep, unsigned long long first, unsigned long long rows,
                 uint32_t* __restrict__ offs, ConstrainTotals* tot) {
  __shared__ uint32_t part[SCAN_THREADS];
  const int t = threadIdx.x;
  const uint32_t nword = (uint32_t)((rows + 63) >> 6);
  const uint32_t per = (nword + SCAN_THREADS - 1) / SCAN_THREADS;
  const uint32_t b = min(nword, (uint32_t)t * per), e = min(nword, b + per);
  uint32_t sum = 0;
  for (uint32_t k = b; k < e; k++) sum += (uint32_t)__popcll(keep[k]);
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < SCAN_THREADS; o <<= 1) {  // inclusive scan of the threads' sums
    const uint32_t v = t >= o ? part[t - o] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;
  for (uint32_t k = b; k < e; k++) {
    offs[k] = run;
    run += (uint32_t)__popcll(keep[k]);
  }
  if (t == 0) {
    const unsigned long long base = tot->base + tot->kept, kept = part[SCAN_THREADS - 1];
    tot->base = base;
    tot->kept = kept;
    tot->move = kept == rows && base == first ? 0ull : 1ull;
  }
}

// The chunk's kept rows -> stage (row k of the chunk's kept rows at stage + shift + k * W), their parent records
// -> stage_par[k].  parents: the level's records (record of level row g at parents[g]).  tr: rows of an LDS tile.
__global__ void __launch_bounds__(64 * CONSTRAIN_WPB)
k_constrain_gather(Ring cur, int W, int tr, unsigned long long first, unsigned long long rows,
                   const unsigned long long* __restrict__ keep, const uint32_t* __restrict__ offs,
                   const unsigned long long* __restrict__ parents, uint32_t* __restrict__ stage,
                   unsigned long long* __restrict__ stage_par, const ConstrainTotals* tot) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  if (!tot->move) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* const tile = lds + wave * tr * W;
  uint32_t* const out = stage + dest_shift(cur, tot->base, W);
  const unsigned long long ngroup = (rows + 63) >> 6;
  for (unsigned long long g = (unsigned long long)blockIdx.x * CONSTRAIN_WPB + wave; g < ngroup;
       g += (unsigned long long)gridDim.x * CONSTRAIN_WPB) {
    const unsigned long long word = keep[g];
    if (!word) continue;
    const unsigned long long row0 = first + (g << 6);  // (a group never wraps the ring)
    const int nv = (int)min<unsigned long long>(64ull, rows - (g << 6));
    unsigned long long k0 = offs[g];
    if (word >> lane & 1) stage_par[k0 + __popcll(word & low_bits(lane))] = parents[row0 + lane];
    for (int r0 = 0; r0 < nv; r0 += tr) {
      const int nt = min(tr, nv - r0);
      const unsigned long long m = word >> r0 & low_bits(nt);
      if (!m) continue;
      copy_words_lds16(tile, ring_row(cur, row0 + r0, W), nt * W, lane);
      wave_sync();
      int nk = 0;
      for (unsigned long long rest = m; rest; rest &= rest - 1, nk++) {  // close the tile's kept rows up, in order
        const int j = __builtin_ctzll(rest);
        if (j == nk) continue;  // (nk < j: the destination ends where the rows not yet moved begin)
        for (int w = lane; w < W; w += 64) tile[nk * W + w] = tile[j * W + w];
        wave_sync();
      }
      store_words_lds(out + k0 * (unsigned long long)W, tile, nk * W, lane);
      k0 += nk;
      wave_sync();  // the next tile's load writes what this store reads
    }
  }
}

// Staging -> the level's rows [base, base + kept) and their parent records.
__global__ void __launch_bounds__(256)
k_constrain_put(Ring cur, int W, const uint32_t* __restrict__ stage, const unsigned long long* __restrict__ stage_par,
                unsigned long long* __restrict__ parents, const ConstrainTotals* tot) {
  if (!tot->move) return;
  const unsigned long long base = tot->base, kept = tot->kept;
  if (!kept) return;
  const uint32_t* const src = stage + dest_shift(cur, base, W);
  const unsigned long long p = ring_idx(cur, base);
  const unsigned long long n1 = min(cur.cap - p, kept);  // rows before the arena's wrap
  copy_words_grid(cur.base + p * (unsigned long long)W, src, n1 * (unsigned long long)W);
  if (kept > n1) copy_words_grid(cur.base, src + n1 * (unsigned long long)W, (kept - n1) * (unsigned long long)W);
  const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (unsigned long long k = tid; k < kept; k += (unsigned long long)gridDim.x * blockDim.x)
    parents[base + k] = stage_par[k];
}

namespace rtla {

hipError_t launch_constrain_pack(const int* masks, uint64_t n, uint64_t* keep, ConstrainTotals* tot, hipStream_t st) {
  if (!n) return hipSuccess;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)device_cus() * 8);
  hipLaunchKernelGGL(k_constrain_pack, dim3(grid), dim3(256), 0, st, masks, (unsigned long long)n,
                     (unsigned long long*)keep, tot);
  return hipGetLastError();
}

hipError_t launch_constrain_move(const Ring& cur, int W, uint64_t first, uint64_t rows, const uint64_t* keep,
                                 uint32_t* offs, uint64_t* parents, uint32_t* stage, uint64_t* stage_par,
                                 ConstrainTotals* tot, hipStream_t st) {
  if (!rows) return hipSuccess;
  if (first % 64 || first + rows > cur.cap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_constrain_scan, dim3(1), dim3(SCAN_THREADS), 0, st, (const unsigned long long*)keep,
                     (unsigned long long)first, (unsigned long long)rows, offs, tot);
  const int tr = audit_tile_rows(W);
  const uint64_t ngroup = (rows + 63) / 64;
  const unsigned ggrid =
      (unsigned)std::min<uint64_t>((ngroup + CONSTRAIN_WPB - 1) / CONSTRAIN_WPB, (uint64_t)device_cus() * 8);
  hipLaunchKernelGGL(k_constrain_gather, dim3(ggrid), dim3(64 * CONSTRAIN_WPB),
                     (size_t)CONSTRAIN_WPB * tr * W * sizeof(uint32_t), st, cur, W, tr, (unsigned long long)first,
                     (unsigned long long)rows, (const unsigned long long*)keep, (const uint32_t*)offs,
                     (const unsigned long long*)parents, stage, (unsigned long long*)stage_par,
                     (const ConstrainTotals*)tot);
  const uint64_t n16 = (rows * (uint64_t)W + 3) / 4;  // 16-byte pieces, four per thread
  const unsigned pgrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n16 + 1023) / 1024, (uint64_t)device_cus() * 8));
  hipLaunchKernelGGL(k_constrain_put, dim3(pgrid), dim3(256), 0, st, cur, W, (const uint32_t*)stage,
                     (const unsigned long long*)stage_par, (unsigned long long*)parents, (const ConstrainTotals*)tot);
  return hipGetLastError();
}

}  // namespace rtla
