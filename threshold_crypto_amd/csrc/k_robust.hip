// gfx950 kernels of the robust combiners (tc_combine_signatures_robust_batch / tc_decrypt_robust_batch): the per-job share
// selection, the gather of the selected shares into the packed operand of the combine kernels, and the verdict that merges
// the two passes (optimistic: the first t+1 present shares; share by share: the first t+1 VALID ones) into status / out /
// used.  Byte shuffling only -- the arithmetic is the combine, hash and pairing kernels' -- in plain C++: every output byte
// has exactly one writer, so there is no atomic and no ordering between lanes.
#include "tc_codec.h"
#include "tc_launch.h"
#include "tc_robust.h"

namespace tc {

// One lane per job: the first `need` eligible slots of the job's N (tc_robust.h select_first).  idx / slot: jobs x need; the
// entries behind the ones found are filled with distinct out-of-range values so that the combine kernels, which run over every
// job, never read an uninitialised abscissa (k_gather_selected gives such a job identities, k_robust_finish fails it).
// used: the B x N bytes of the CALLER's job numbering -- map[j] is job j's row there (null: j) -- set for the selected slots
// of a job that has enough, untouched otherwise.  enough[j] = 1 iff `need` slots were found.
__global__ void k_select_shares(const uint8_t* __restrict__ present, const uint8_t* __restrict__ bad, size_t N, size_t need, size_t jobs,
                                const uint32_t* __restrict__ map, uint64_t* __restrict__ idx, uint32_t* __restrict__ slot,
                                uint8_t* __restrict__ used, uint8_t* __restrict__ enough) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= jobs) return;
  uint64_t* my_idx = idx + j * need;
  uint32_t* my_slot = slot + j * need;
  const size_t count = select_first(present ? present + j * N : nullptr, bad ? bad + j * N : nullptr, N, need, my_idx, my_slot);
  for (size_t k = count; k < need; k++) {
    my_idx[k] = (uint64_t)(N + k);
    my_slot[k] = 0xffffffffu;
  }
  const bool full = count == need;
  enough[j] = full ? 1 : 0;
  if (used && full) {
    uint8_t* row = used + (size_t)(map ? map[j] : (uint32_t)j) * N;
    for (size_t k = 0; k < need; k++) row[my_slot[k]] = 1;
  }
}

// dst[(j * need + k) * PB ..] = shares[(j * N + slot[j * need + k]) * PB ..]: one lane per V (16 bytes; 8 when a buffer is
// only 8-byte aligned) of output, consecutive lanes on consecutive words of a row, so a wave reads and writes whole rows.  A
// job without enough shares gets the identity's encoding (0x40, then zeros) in every position: decodable input for the
// combine kernel, whose result k_robust_finish discards.
template <class V>
__global__ void k_gather_selected(const uint8_t* __restrict__ shares, size_t N, size_t need, size_t row_words, const uint32_t* __restrict__ slot,
                                  const uint8_t* __restrict__ enough, size_t jobs, uint8_t* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= jobs * need * row_words) return;
  const size_t rec = i / row_words, w = i % row_words;
  const size_t j = rec / need;
  V val;
  if (enough[j]) {
    val = reinterpret_cast<const V*>(shares)[(j * N + (size_t)slot[rec]) * row_words + w];
  } else {
    val = V{};
    if (w == 0) val.x = 0x40;  // byte 0 of the row (little-endian lanes)
  }
  reinterpret_cast<V*>(dst)[i] = val;
}

// dst[r] = src[map[r]]: a per-job byte for every record of the share-by-share pass
__global__ void k_gather_bytes(const uint8_t* __restrict__ src, const uint32_t* __restrict__ map, size_t rows, uint8_t* __restrict__ dst) {
  const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (r < rows) dst[r] = src[map[r]];
}

// The share-by-share verdicts.  Record r is share rec[r] = job * N + i of the caller's arrays; ok[r] its pairing check (and
// membership).  c_present / c_bad: the compacted masks the second selection reads; bad[rec[r]] (optional) the caller's.  An
// absent slot is neither: whatever its bytes decoded to is dropped here.
__global__ void k_robust_mark(const uint8_t* __restrict__ present, const uint32_t* __restrict__ rec, const uint8_t* __restrict__ ok, size_t rows,
                              uint8_t* __restrict__ c_present, uint8_t* __restrict__ c_bad, uint8_t* __restrict__ bad) {
  const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  const uint32_t src = rec[r];
  const uint8_t p = (!present || present[src] != 0) ? 1 : 0;
  const uint8_t b = (p && ok[r] == 0) ? 1 : 0;
  c_present[r] = p;
  c_bad[r] = b;
  if (bad) bad[src] = b;
}

// The verdict of one pass, row_words lanes per job (one per 8 bytes of the point result: the caller's output buffer is only
// promised to be 8-byte aligned).  Job f of the pass is job map[f]
// of the call (null: f).  Its combination stands when it had enough shares, the combine kernel decoded them all (st), the
// check of the combination passed (ok; null: the shares were checked one by one, nothing to add) and every selected share is
// a group member (member: need bytes per job, or null).  Then status OK and the combination; otherwise NOT_ENOUGH_SHARES, the
// identity and a cleared `used` row -- for a job of the first pass that only lacked validity (verdict kRobustRetry) that is
// the answer the second pass overwrites if it finds t+1 valid shares.
__global__ void k_robust_finish(const uint32_t* __restrict__ map, size_t N, size_t need, size_t row_words, size_t jobs,
                                const uint8_t* __restrict__ enough, const uint8_t* __restrict__ st, const uint8_t* __restrict__ ok,
                                const uint8_t* __restrict__ member, const uint8_t* __restrict__ comb, uint8_t* __restrict__ out,
                                uint8_t* __restrict__ status, uint8_t* __restrict__ used, uint8_t* __restrict__ verdict) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= jobs * row_words) return;
  const size_t f = i / row_words, w = i % row_words;
  const size_t job = map ? map[f] : f;
  const bool full = enough[f] != 0;
  bool good = full && st[f] == TC_JOB_OK && (!ok || ok[f] != 0);
  if (good && member)
    for (size_t k = 0; k < need; k++) good = good && member[f * need + k] != 0;
  uint2 val;
  if (good) {
    val = reinterpret_cast<const uint2*>(comb)[i];
  } else {
    val = uint2{};
    if (w == 0) val.x = 0x40;
  }
  reinterpret_cast<uint2*>(out)[job * row_words + w] = val;
  if (used && full && !good)  // (a job without enough shares never had a byte set)
    for (size_t k = w; k < N; k += row_words) used[job * N + k] = 0;
  if (w == 0) {
    status[job] = good ? TC_JOB_OK : TC_JOB_NOT_ENOUGH_SHARES;
    if (verdict) verdict[f] = good ? kRobustGood : (full ? kRobustRetry : kRobustNotEnough);
  }
}

void launch_select_shares(hipStream_t st, const uint8_t* present, const uint8_t* bad, size_t N, size_t need, size_t jobs, const uint32_t* map,
                          uint64_t* idx, uint32_t* slot, uint8_t* used, uint8_t* enough) {
  if (jobs) hipLaunchKernelGGL(k_select_shares, dim3(grid_for(jobs)), dim3(kBlock), 0, st, present, bad, N, need, jobs, map, idx, slot, used, enough);
}

void launch_gather_selected(hipStream_t st, const uint8_t* shares, size_t N, size_t need, size_t point_bytes, const uint32_t* slot,
                            const uint8_t* enough, size_t jobs, uint8_t* dst) {
  if (!jobs || !need) return;
  // (the caller's share array is only promised to be 8-byte aligned in device-I/O mode)
  if (((((uintptr_t)shares) | ((uintptr_t)dst)) & 15) == 0) {
    const size_t rw = point_bytes / 16;
    hipLaunchKernelGGL(k_gather_selected<uint4>, dim3(grid_for(jobs * need * rw)), dim3(kBlock), 0, st, shares, N, need, rw, slot, enough, jobs, dst);
  } else {
    const size_t rw = point_bytes / 8;
    hipLaunchKernelGGL(k_gather_selected<uint2>, dim3(grid_for(jobs * need * rw)), dim3(kBlock), 0, st, shares, N, need, rw, slot, enough, jobs, dst);
  }
}

void launch_gather_bytes(hipStream_t st, const uint8_t* src, const uint32_t* map, size_t rows, uint8_t* dst) {
  if (rows) hipLaunchKernelGGL(k_gather_bytes, dim3(grid_for(rows)), dim3(kBlock), 0, st, src, map, rows, dst);
}

void launch_robust_mark(hipStream_t st, const uint8_t* present, const uint32_t* rec, const uint8_t* ok, size_t rows, uint8_t* c_present,
                        uint8_t* c_bad, uint8_t* bad) {
  if (rows) hipLaunchKernelGGL(k_robust_mark, dim3(grid_for(rows)), dim3(kBlock), 0, st, present, rec, ok, rows, c_present, c_bad, bad);
}

void launch_robust_finish(hipStream_t st, const uint32_t* map, size_t N, size_t need, size_t point_bytes, size_t jobs, const uint8_t* enough,
                          const uint8_t* job_st, const uint8_t* ok, const uint8_t* member, const uint8_t* comb, uint8_t* out, uint8_t* status,
                          uint8_t* used, uint8_t* verdict) {
  const size_t rw = point_bytes / 8;
  if (jobs)
    hipLaunchKernelGGL(k_robust_finish, dim3(grid_for(jobs * rw)), dim3(kBlock), 0, st, map, N, need, rw, jobs, enough, job_st, ok, member, comb, out,
                       status, used, verdict);
}

}  // namespace tc
