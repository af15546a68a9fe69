// gfx950 kernels: G2 linear combinations in two stages (tc_msm.h) -- the share combiner of the general path (every
// job the small-index fast path does not take; BASELINE config "t=67, N=200") and tc_g2_lincomb_batch.
#include "tc_msm.h"
#include "tc_records.h"
#include "tc_launch.h"

namespace tc {

// which jobs of the batch are this path's: all of them, or (share combination with t <= 3) those the small-index fast
// path of k_combine_fast leaves alone; *need counts them (k_lagrange) and zero ends the kernel at once
__device__ __forceinline__ bool msm_job_taken(const MsmFilter& f, size_t j) {
  return !(f.idx && f.t >= 1 && f.t <= 3 && combine_small_applies(f.idx + j * f.n_per_job, (int)f.t));
}

// stage T: one lane pair per (job, chunk of 4 shares)
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_msm_tables(size_t n, size_t pts_stride, const uint8_t* __restrict__ points,
                                                                  const uint32_t* __restrict__ scalars, size_t B,
                                                                  int32_t* __restrict__ tbl, uint8_t* __restrict__ codes,
                                                                  uint8_t* __restrict__ status, int nbits, MsmFilter f) {
  if (f.need && *f.need == 0) return;
  const size_t chunks = msm_chunks(n);
  const size_t tid = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  if (tid >= B * chunks) return;
  const size_t j = tid / chunks, c = tid % chunks;
  if (!msm_job_taken(f, j)) return;
  const size_t shares4 = chunks * kMsmChunk;
  const bool ok = job_msm_tables(n, c, points + j * pts_stride, scalars + j * n * 8, tbl + j * shares4 * 8 * kMsmEntryWords,
                                 codes + j * kMsmColumns * shares4, pair_leader(), nbits);
  if (!ok && pair_leader() && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
}

// stage L: one lane pair per job
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_msm_ladder(size_t n, size_t B, const int32_t* __restrict__ tbl,
                                                                  const uint8_t* __restrict__ codes, uint8_t* __restrict__ out,
                                                                  const uint8_t* __restrict__ status, int nbits, MsmFilter f) {
  if (f.need && *f.need == 0) return;
  const size_t j = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  if (j >= B) return;
  if (!msm_job_taken(f, j)) return;
  if (status[j] != TC_JOB_OK) {
    g2_encode_uncompressed(G2Affine::infinity(), out + j * 192);
    return;
  }
  const size_t shares4 = msm_chunks(n) * kMsmChunk;
  const G2Jac r = job_msm_ladder(n, tbl + j * shares4 * 8 * kMsmEntryWords, codes + j * kMsmColumns * shares4, nbits);
  g2_encode_uncompressed(jac_to_affine(r), out + j * 192);
}
// stage L for batches that would not fill the GPU with one lane pair per job: `parts` (a power of two, 2 .. 32) lane
// pairs per job, each over a range of the job's shares (tc_msm.h msm_part); the partial sums are added across the lane
// pairs of the job (they sit in one wave) in log2(parts) rounds, the first one writes the result.
__device__ __forceinline__ Fq2 msm_from_partner(const Fq2& v, int lanes) {
  Fq2 r = v;
  TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) r.m.l[i] = __shfl_xor(v.m.l[i], lanes, 64);
  return r;
}
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_msm_ladder_split(size_t n, size_t B, const int32_t* __restrict__ tbl,
                                                                        const uint8_t* __restrict__ codes, uint8_t* __restrict__ out,
                                                                        const uint8_t* __restrict__ status, int nbits, MsmFilter f,
                                                                        size_t parts) {
  if (f.need && *f.need == 0) return;
  const size_t lp = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const size_t j = lp / parts, g = lp % parts;
  if (j >= B) return;
  if (!msm_job_taken(f, j)) return;
  if (status[j] != TC_JOB_OK) {
    if (g == 0) g2_encode_uncompressed(G2Affine::infinity(), out + j * 192);
    return;
  }
  const size_t shares4 = msm_chunks(n) * kMsmChunk;
  G2Jac r = job_msm_ladder_part<true>(n, tbl + j * shares4 * 8 * kMsmEntryWords, codes + j * kMsmColumns * shares4, nbits, msm_part(n, g, parts));
  TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
    const int lanes = (int)(d * kG2Lanes);
    const G2Jac o{msm_from_partner(r.x, lanes), msm_from_partner(r.y, lanes), msm_from_partner(r.z, lanes)};
    r = jac_add(r, o);
  }
  if (g == 0) g2_encode_uncompressed(jac_to_affine(r), out + j * 192);
}

// ONE point set shared by every job with short scalars (the recoding never negates a base then): one table set for the launch
__host__ __device__ inline bool msm_g1_shared_tables(size_t pts_stride, int nbits) { return pts_stride == 0 && nbits < 128; }
// ---- G1 (tc_msm.h): stage T one lane per (job, chunk of 4 shares), stage L one lane per job -- or per PART of a job
// when the batch alone does not fill the GPU (a job's `parts` lanes are adjacent; their partial sums meet in
// log2(parts) rounds of one __shfl_xor exchange + one addition).  Two waves per SIMD (256 registers).
__global__ __launch_bounds__(kBlock, 2) void k_msm_tables_g1(size_t n, size_t pts_stride, const uint8_t* __restrict__ points,
                                                           const uint32_t* __restrict__ scalars, size_t B, int32_t* __restrict__ tbl,
                                                           uint8_t* __restrict__ codes, uint8_t* __restrict__ status, int nbits) {
  const size_t chunks = msm_chunks(n);
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (tid >= B * chunks) return;
  const size_t j = tid / chunks, c = tid % chunks;
  const size_t shares4 = chunks * kMsmChunk;
  // ONE point set shared by every job, short scalars (the random linear combinations of the RLC checks): one table set, built
  // by job 0; the other jobs only recode their scalars (B x N x 1 KiB of identical tables before)
  const bool shared = msm_g1_shared_tables(pts_stride, nbits);
  const bool ok = job_msm_tables_g1(n, c, points + j * pts_stride, scalars + j * n * 8, tbl + (shared ? 0 : j * shares4 * 8 * kMsmEntryWordsG1),
                                    codes + j * kMsmColumns * shares4, nbits, !shared || j == 0);
  if (!ok && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
}
__device__ __forceinline__ Fq msm_from_lane(const Fq& v, int lanes) {
  Fq r = v;
  TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) r.l[i] = __shfl_xor(v.l[i], lanes, 64);
  return r;
}
template <bool SPLIT>
__global__ __launch_bounds__(kBlock, 2) void k_msm_ladder_g1(size_t n, size_t B, const int32_t* __restrict__ tbl, const uint8_t* __restrict__ codes,
                                                           uint8_t* __restrict__ out, const uint8_t* __restrict__ status, size_t parts, int top,
                                                           int shared) {
  const size_t lp = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t j = lp / parts, g = lp % parts;
  if (j >= B) return;  // (parts divides 64: a job's lanes leave together)
  if (status[j] != TC_JOB_OK) {
    if (g == 0) g1_encode_uncompressed(G1Affine::infinity(), out + j * 96);
    return;
  }
  const size_t shares4 = msm_chunks(n) * kMsmChunk;
  G1Jac r = job_msm_ladder_g1_part<SPLIT>(n, tbl + (shared ? 0 : j * shares4 * 8 * kMsmEntryWordsG1), codes + j * kMsmColumns * shares4,
                                          msm_part(n, g, parts), top);
  if (SPLIT) {
    TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
      const G1Jac o{msm_from_lane(r.x, (int)d), msm_from_lane(r.y, (int)d), msm_from_lane(r.z, (int)d)};
      r = jac_add(r, o);
    }
  }
  if (g == 0) g1_encode_uncompressed(jac_to_affine(r), out + j * 96);
}

size_t msm_table_bytes_g1(size_t n, size_t B) { return B * msm_chunks(n) * kMsmChunk * 8 * kMsmEntryWordsG1 * sizeof(int32_t); }
// jobs that own a table set in a launch_msm_g1 call: all of them, or one for a shared point set in short-scalar mode
size_t msm_table_jobs_g1(size_t pts_stride, int nbits, size_t B) { return msm_g1_shared_tables(pts_stride, nbits) ? 1 : B; }
// status: B bytes, TC_JOB_OK for the jobs to run (others get the identity and keep their status)
// nbits = 128: any scalars below r.  nbits < 128 (even): odd scalars k1 + k2 x^2 with k1, k2 < 2^nbits (a job with another
// scalar fails): nbits doublings instead of 128.
void launch_msm_g1(hipStream_t st, size_t n, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, size_t B, int32_t* tbl,
                   uint8_t* codes, uint8_t* out, uint8_t* status, int nbits) {
  if (!B || !n) return;
  const int top = nbits / 2;
  const int shared = msm_g1_shared_tables(pts_stride, nbits) ? 1 : 0;
  hipLaunchKernelGGL(k_msm_tables_g1, dim3(grid_for(B * msm_chunks(n))), dim3(kBlock), 0, st, n, pts_stride, points, scalars, B, tbl, codes, status, nbits);
  // lanes per job in stage L: 1 when the batch fills the 2048 wave slots by itself (131 072 lanes), else the power of two
  // that does, with at least four shares per part
  size_t parts = 1;
  while (parts < 64 && B * parts * 2 <= 131072 && parts * 2 * 4 <= n) parts *= 2;
  if (parts == 1)
    hipLaunchKernelGGL(k_msm_ladder_g1<false>, dim3(grid_for(B)), dim3(kBlock), 0, st, n, B, (const int32_t*)tbl, (const uint8_t*)codes, out,
                       (const uint8_t*)status, parts, top, shared);
  else
    hipLaunchKernelGGL(k_msm_ladder_g1<true>, dim3(grid_for(B * parts)), dim3(kBlock), 0, st, n, B, (const int32_t*)tbl, (const uint8_t*)codes, out,
                       (const uint8_t*)status, parts, top, shared);
}

size_t msm_table_bytes(size_t n, size_t B) { return B * msm_chunks(n) * kMsmChunk * 8 * kMsmEntryWords * sizeof(int32_t); }
size_t msm_code_bytes(size_t n, size_t B) { return B * kMsmColumns * msm_chunks(n) * kMsmChunk; }
// status: B bytes, TC_JOB_OK for the jobs to run (others get the identity and keep their status)
// nbits = 64: any scalars below r.  nbits < 64: odd scalars whose four base-|x| digits are below 2^nbits (a job with
// another scalar fails): nbits doublings instead of 64.
void launch_msm_g2(hipStream_t st, size_t n, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, size_t B,
                   int32_t* tbl, uint8_t* codes, uint8_t* out, uint8_t* status, int nbits, MsmFilter f) {
  if (!B || !n) return;
  const size_t lanes = B * msm_chunks(n) * kG2Lanes;
  hipLaunchKernelGGL(k_msm_tables, dim3(grid_for(lanes)), dim3(kBlock), 0, st, n, pts_stride, points, scalars, B, tbl, codes, status, nbits, f);
  // lane pairs per job in stage L: 1 when the batch fills the GPU's 2048 wave slots by itself (65 536 lane pairs), else
  // the power of two that does, with at least four shares per part
  size_t parts = 1;
  while (parts < 32 && B * parts * 2 <= 65536 && parts * 2 * 4 <= n) parts *= 2;
  if (parts == 1)
    hipLaunchKernelGGL(k_msm_ladder, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, n, B, (const int32_t*)tbl, (const uint8_t*)codes, out,
                       (const uint8_t*)status, nbits, f);
  else
    hipLaunchKernelGGL(k_msm_ladder_split, dim3(grid_for(B * parts * kG2Lanes)), dim3(kBlock), 0, st, n, B, (const int32_t*)tbl,
                       (const uint8_t*)codes, out, (const uint8_t*)status, nbits, f, parts);
}

// ---- ragged sums (tc_records.h; tc_verify_g2_records_rlc_batch) -----------------------------------------------
// The same two stages over SEGMENTS of one record array: segment j owns the records seg_first[j] .. seg_first[j + 1] and the
// chunks first_chunk[j] .. first_chunk[j + 1] (both arrays J + 1 values, made by the host: rec_chunk_ranges).  Its tables and
// codes have the layout of a job of the fixed-n kernels with n = its length, so stage T and stage L are job_msm_tables* /
// job_msm_ladder*_part as they are; what is new is where a lane finds its work.
static_assert(kRecChunk == kMsmChunk, "tc_records.h pads segments to the chunk of the two-stage kernels");

// keys[r] = pks[key_idx[r]] (six lanes per record, 16 bytes each); an index outside the table leaves 96 bytes that no decoder
// accepts (flag bit 7), so the record's segment fails in stage T and the record in the per-record pass
__global__ __launch_bounds__(kBlock) void k_rec_gather_keys(const uint8_t* __restrict__ pks, size_t K, const uint64_t* __restrict__ key_idx, size_t R,
                                                          uint8_t* __restrict__ keys) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t r = tid / 6, w = tid % 6;
  if (r >= R) return;
  const uint64_t i = key_idx[r];
  uint8_t* dst = keys + r * 96 + w * 16;
  if (i < K) {
    const uint8_t* src = pks + (size_t)i * 96 + w * 16;
    for (int b = 0; b < 16; b++) dst[b] = src[b];
  } else {
    for (int b = 0; b < 16; b++) dst[b] = 0xff;
  }
}

// the longest trip count among the lanes of the wave (every lane of the wave calls it)
__device__ __forceinline__ uint32_t rec_wave_max(uint32_t v) {
  TC_UNROLL for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// stage T: one lane pair per chunk of the launch, whichever segment it belongs to
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_rec_tables_g2(const uint8_t* __restrict__ points, const uint32_t* __restrict__ scalars,
                                                                     const uint64_t* __restrict__ seg_first, const uint64_t* __restrict__ first_chunk,
                                                                     size_t J, int32_t* __restrict__ tbl, uint8_t* __restrict__ codes,
                                                                     uint8_t* __restrict__ status, int nbits) {
  const uint64_t c = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  if (c >= first_chunk[J]) return;
  const size_t j = rec_segment_of_chunk(first_chunk, J, c);
  const uint64_t r0 = seg_first[j], len = seg_first[j + 1] - r0, p0 = first_chunk[j] * kMsmChunk;
  const bool ok = job_msm_tables((size_t)len, (size_t)(c - first_chunk[j]), points + r0 * 192, scalars + r0 * 8, tbl + p0 * 8 * kMsmEntryWords,
                                 codes + p0 * kMsmColumns, pair_leader(), nbits);
  if (!ok && pair_leader() && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
}

// stage L: `parts` lane pairs per segment (a power of two <= 32), each over rec_part's share of the segment's records.  The
// segments of a wave differ in length: every lane runs the look-ups of the LONGEST part in the wave (one trip count per wave,
// tc_common.h wave_any) and masks the ones past its own end.  A part without records -- an empty segment, a segment shorter
// than `parts`, a segment that failed in stage T -- runs the loop over place 0 (of its segment, or of the launch), which exists
// whenever the launch has a record, and its sum is replaced by the identity.  No lane of a live segment leaves before the last
// exchange; the lanes behind the last segment leave as whole segments, after the wave's trip count is agreed.
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_rec_ladder_g2(const uint64_t* __restrict__ seg_first, const uint64_t* __restrict__ first_chunk,
                                                                     size_t J, const int32_t* __restrict__ tbl, const uint8_t* __restrict__ codes,
                                                                     uint8_t* __restrict__ out, const uint8_t* __restrict__ status, int nbits,
                                                                     size_t parts) {
  const size_t lp = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const size_t j = lp / parts, g = lp % parts;
  const bool live = j < J;
  uint64_t len = 0, p0 = 0;
  if (live && status[j] == TC_JOB_OK) {
    len = seg_first[j + 1] - seg_first[j];
    p0 = len ? first_chunk[j] * kMsmChunk : 0;
  }
  const uint32_t trips = rec_wave_max((uint32_t)rec_part_trips(len, parts));
  if (!live) return;
  const RecPart rp = rec_part(len, g, parts);
  const bool none = rp.s0 >= rp.s1;
  G2Jac r = job_msm_ladder_part<true>(len ? (size_t)len : 1, tbl + p0 * 8 * kMsmEntryWords, codes + p0 * kMsmColumns, nbits,
                                      MsmPart{(size_t)rp.s0, (size_t)rp.s1, (size_t)trips});
  r = G2Jac::select(none, G2Jac::infinity(), r);
  TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
    const int lanes = (int)(d * kG2Lanes);
    const G2Jac o{msm_from_partner(r.x, lanes), msm_from_partner(r.y, lanes), msm_from_partner(r.z, lanes)};
    r = jac_add(r, o);
  }
  if (g == 0) g2_encode_uncompressed(jac_to_affine(r), out + j * 192);
}

// the same in G1: one lane per chunk, `parts` lanes per segment (a power of two <= 64)
__global__ __launch_bounds__(kBlock, 2) void k_rec_tables_g1(const uint8_t* __restrict__ points, const uint32_t* __restrict__ scalars,
                                                           const uint64_t* __restrict__ seg_first, const uint64_t* __restrict__ first_chunk, size_t J,
                                                           int32_t* __restrict__ tbl, uint8_t* __restrict__ codes, uint8_t* __restrict__ status,
                                                           int nbits) {
  const uint64_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= first_chunk[J]) return;
  const size_t j = rec_segment_of_chunk(first_chunk, J, c);
  const uint64_t r0 = seg_first[j], len = seg_first[j + 1] - r0, p0 = first_chunk[j] * kMsmChunk;
  const bool ok = job_msm_tables_g1((size_t)len, (size_t)(c - first_chunk[j]), points + r0 * 96, scalars + r0 * 8, tbl + p0 * 8 * kMsmEntryWordsG1,
                                    codes + p0 * kMsmColumns, nbits, true);
  if (!ok && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
}
__global__ __launch_bounds__(kBlock, 2) void k_rec_ladder_g1(const uint64_t* __restrict__ seg_first, const uint64_t* __restrict__ first_chunk, size_t J,
                                                           const int32_t* __restrict__ tbl, const uint8_t* __restrict__ codes, uint8_t* __restrict__ out,
                                                           const uint8_t* __restrict__ status, int top, size_t parts) {
  const size_t lp = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t j = lp / parts, g = lp % parts;
  const bool live = j < J;
  uint64_t len = 0, p0 = 0;
  if (live && status[j] == TC_JOB_OK) {
    len = seg_first[j + 1] - seg_first[j];
    p0 = len ? first_chunk[j] * kMsmChunk : 0;
  }
  const uint32_t trips = rec_wave_max((uint32_t)rec_part_trips(len, parts));
  if (!live) return;
  const RecPart rp = rec_part(len, g, parts);
  const bool none = rp.s0 >= rp.s1;
  G1Jac r = job_msm_ladder_g1_part<true>(len ? (size_t)len : 1, tbl + p0 * 8 * kMsmEntryWordsG1, codes + p0 * kMsmColumns,
                                         MsmPart{(size_t)rp.s0, (size_t)rp.s1, (size_t)trips}, top);
  r = G1Jac::select(none, G1Jac::infinity(), r);
  TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
    const G1Jac o{msm_from_lane(r.x, (int)d), msm_from_lane(r.y, (int)d), msm_from_lane(r.z, (int)d)};
    r = jac_add(r, o);
  }
  if (g == 0) g1_encode_uncompressed(jac_to_affine(r), out + j * 96);
}

// The PAIRED form (tc_verify_decryption_share_records_rlc_batch): segment j is summed over points_a AND over
// points_b with the same scalars, both in one launch per stage (tc_records.h rec_pair_*: where a lane finds its work).  Half 1
// keeps tables and digit codes of its own behind half 0's; the bodies are job_msm_tables_g1 / job_msm_ladder_g1_part as they are.
// status[j] is set when either half fails.
__global__ __launch_bounds__(kBlock, 2) void k_rec_tables_g1_pair(const uint8_t* __restrict__ points_a, const uint8_t* __restrict__ points_b,
                                                                const uint32_t* __restrict__ scalars, const uint64_t* __restrict__ seg_first,
                                                                const uint64_t* __restrict__ first_chunk, size_t J, int32_t* __restrict__ tbl,
                                                                uint8_t* __restrict__ codes, uint8_t* __restrict__ status, int nbits) {
  const uint64_t t = (size_t)blockIdx.x * kBlock + threadIdx.x, chunks = first_chunk[J];
  if (t >= rec_pair_tables_lanes(chunks)) return;
  const RecPairChunk h = rec_pair_chunk(t, chunks);
  const size_t j = rec_segment_of_chunk(first_chunk, J, h.c);
  const uint64_t r0 = seg_first[j], len = seg_first[j + 1] - r0, p0 = rec_pair_place(h.half, first_chunk[j], chunks);
  const bool ok = job_msm_tables_g1((size_t)len, (size_t)(h.c - first_chunk[j]), (h.half ? points_b : points_a) + r0 * 96, scalars + r0 * 8,
                                    tbl + p0 * 8 * kMsmEntryWordsG1, codes + p0 * kMsmColumns, nbits, true);
  if (!ok && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
}
// stage L: the rules of k_rec_ladder_g1 (one trip count per wave, masked look-ups, the identity for a part without records, no
// lane of a live sum leaving before the last exchange) over 2 J sums; the leader lane of a sum writes A_j, or -B_j, into the
// interleaved operand array of the product check (the identity stays the identity: its encoding has no y)
__global__ __launch_bounds__(kBlock, 2) void k_rec_ladder_g1_pair(const uint64_t* __restrict__ seg_first, const uint64_t* __restrict__ first_chunk,
                                                                size_t J, const int32_t* __restrict__ tbl, const uint8_t* __restrict__ codes,
                                                                uint8_t* __restrict__ out, const uint8_t* __restrict__ status, int top, size_t parts) {
  const RecPairLane w = rec_pair_lane((size_t)blockIdx.x * kBlock + threadIdx.x, parts);
  const bool live = w.j < J;
  uint64_t len = 0, p0 = 0;
  if (live && status[w.j] == TC_JOB_OK) {
    len = seg_first[w.j + 1] - seg_first[w.j];
    p0 = len ? rec_pair_place(w.half, first_chunk[w.j], first_chunk[J]) : 0;
  }
  const uint32_t trips = rec_wave_max((uint32_t)rec_part_trips(len, parts));
  if (!live) return;
  const RecPart rp = rec_part(len, w.g, parts);
  const bool none = rp.s0 >= rp.s1;
  G1Jac r = job_msm_ladder_g1_part<true>(len ? (size_t)len : 1, tbl + p0 * 8 * kMsmEntryWordsG1, codes + p0 * kMsmColumns,
                                         MsmPart{(size_t)rp.s0, (size_t)rp.s1, (size_t)trips}, top);
  r = G1Jac::select(none, G1Jac::infinity(), r);
  TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
    const G1Jac o{msm_from_lane(r.x, (int)d), msm_from_lane(r.y, (int)d), msm_from_lane(r.z, (int)d)};
    r = jac_add(r, o);
  }
  if (w.g == 0) {
    G1Affine a = jac_to_affine(r);
    a.y = Fq::select(w.half != 0, -a.y, a.y).norm();
    g1_encode_uncompressed(a, out + rec_pair_out(w.j, w.half));
  }
}

size_t rec_table_bytes(bool g2, uint64_t chunks) {
  return (size_t)chunks * kMsmChunk * 8 * (g2 ? kMsmEntryWords : kMsmEntryWordsG1) * sizeof(int32_t);
}
size_t rec_code_bytes(uint64_t chunks) { return (size_t)chunks * kMsmChunk * kMsmColumns; }
void launch_rec_gather_keys(hipStream_t st, const uint8_t* pks, size_t K, const uint64_t* key_idx, size_t R, uint8_t* keys) {
  if (!R) return;
  hipLaunchKernelGGL(k_rec_gather_keys, dim3(grid_for(R * 6)), dim3(kBlock), 0, st, pks, K, key_idx, R, keys);
}
// out[j] = sum_r scalars[r] points[r] over segment j's records, J segments with `chunks` = first_chunk[J] >= 1 chunks in all.
// status: J bytes (TC_JOB_OK to run; a segment with an undecodable point or a scalar that is not short gets
// TC_JOB_INVALID_ENCODING and the identity).  nbits: the short-scalar modes of launch_msm_g2 (< 64) / launch_msm_g1 (< 128, even).
void launch_rec_sum_g2(hipStream_t st, const uint8_t* points, const uint32_t* scalars, const uint64_t* seg_first, const uint64_t* first_chunk, size_t J,
                       uint64_t chunks, size_t parts, int32_t* tbl, uint8_t* codes, uint8_t* out, uint8_t* status, int nbits) {
  if (!J || !chunks) return;
  if (parts < 1 || parts > (size_t)kBlock / kG2Lanes || (parts & (parts - 1))) parts = 1;
  hipLaunchKernelGGL(k_rec_tables_g2, dim3(grid_for((size_t)chunks * kG2Lanes)), dim3(kBlock), 0, st, points, scalars, seg_first, first_chunk, J, tbl,
                     codes, status, nbits);
  hipLaunchKernelGGL(k_rec_ladder_g2, dim3(grid_for(J * parts * kG2Lanes)), dim3(kBlock), 0, st, seg_first, first_chunk, J, (const int32_t*)tbl,
                     (const uint8_t*)codes, out, (const uint8_t*)status, nbits, parts);
}
void launch_rec_sum_g1(hipStream_t st, const uint8_t* points, const uint32_t* scalars, const uint64_t* seg_first, const uint64_t* first_chunk, size_t J,
                       uint64_t chunks, size_t parts, int32_t* tbl, uint8_t* codes, uint8_t* out, uint8_t* status, int nbits) {
  if (!J || !chunks) return;
  if (parts < 1 || parts > (size_t)kBlock || (parts & (parts - 1))) parts = 1;
  hipLaunchKernelGGL(k_rec_tables_g1, dim3(grid_for((size_t)chunks)), dim3(kBlock), 0, st, points, scalars, seg_first, first_chunk, J, tbl, codes, status,
                     nbits);
  hipLaunchKernelGGL(k_rec_ladder_g1, dim3(grid_for(J * parts)), dim3(kBlock), 0, st, seg_first, first_chunk, J, (const int32_t*)tbl,
                     (const uint8_t*)codes, out, (const uint8_t*)status, nbits / 2, parts);
}
// out[2 j] = sum_r scalars[r] points_a[r], out[2 j + 1] = -sum_r scalars[r] points_b[r] over segment j's records (J x 2 x 96
// bytes: the a operands of launch_pairing_product_check with two pairs per segment), ONE launch per stage for both sums.
// tbl: rec_table_bytes(false, 2 chunks), codes: rec_code_bytes(2 chunks); status: J bytes, set when either half fails.
void launch_rec_sum_g1_pair(hipStream_t st, const uint8_t* points_a, const uint8_t* points_b, const uint32_t* scalars, const uint64_t* seg_first,
                            const uint64_t* first_chunk, size_t J, uint64_t chunks, size_t parts, int32_t* tbl, uint8_t* codes, uint8_t* out,
                            uint8_t* status, int nbits) {
  if (!J || !chunks) return;
  if (parts < 1 || parts > (size_t)kBlock || (parts & (parts - 1))) parts = 1;
  hipLaunchKernelGGL(k_rec_tables_g1_pair, dim3(grid_for((size_t)rec_pair_tables_lanes(chunks))), dim3(kBlock), 0, st, points_a, points_b, scalars,
                     seg_first, first_chunk, J, tbl, codes, status, nbits);
  hipLaunchKernelGGL(k_rec_ladder_g1_pair, dim3(grid_for(rec_pair_ladder_lanes(J, parts))), dim3(kBlock), 0, st, seg_first, first_chunk, J,
                     (const int32_t*)tbl, (const uint8_t*)codes, out, (const uint8_t*)status, nbits / 2, parts);
}

}  // namespace tc
