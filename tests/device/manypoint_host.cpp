// Host leg of the many-point conformance harness (tests/manypoint_conformance.py): the header routines the kernels of
// k_msm.hip / k_comb.hip call -- job_msm_tables, job_msm_ladder_part<SPLIT>, their G1 twins, job_comb_tables, job_comb_sign,
// job_comb_tables_g1, job_comb_decrypt, the lane arithmetic of the ragged and the paired ragged sums (tc_records.h), and the
// routines of k_blame.hip (tc_blame_jobs.h: blame_call_seed, job_blame_leaf, blame_leaf_g1 / _g2, job_blame_range_part) --
// run by g++ with -DTC_BOUND_CHECK over the same buffers, in the layout of tests/device/manypoint.hip: the jobs one after the
// other, the parts of a job one after the other, then the kernel's xor tree of jac_add.  It proves the case tables, the
// models and the checkers before any GPU time is spent.  What it cannot see is the kernels' own text (lane pairs, the
// shuffle merge, the indexing): that is the GPU leg.  parts / share = 0 (the launcher's choice) exists on the device only.
// With -DMP_MAIN it is a stand-alone program over a fixed short case list (for a g++ -fsanitize=address,undefined build).
// Test code only: never linked into libtc_amd.so.
#include "../../threshold_crypto_amd/csrc/tc_msm.h"
#include "../../threshold_crypto_amd/csrc/tc_comb.h"
#include "../../threshold_crypto_amd/csrc/tc_comb_g1.h"
#include "../../threshold_crypto_amd/csrc/tc_records.h"
#include "../../threshold_crypto_amd/csrc/tc_blame_jobs.h"

#include <stdio.h>
#include <string.h>
#include <type_traits>
#include <vector>

using namespace tc;

namespace {
bool taken(const uint64_t* idx, size_t n_per_job, size_t t, size_t j) {
  return !(idx && t >= 1 && t <= 3 && combine_small_applies(idx + j * n_per_job, (int)t));
}
template <class J>
J merge(std::vector<J> r, size_t parts) {
  for (size_t d = 1; d < parts; d <<= 1) {  // every lane (pair) adds its partner's value of the round before
    std::vector<J> nr(parts);
    for (size_t g = 0; g < parts; g++) nr[g] = jac_add(r[g], r[g ^ d]);
    r = nr;
  }
  return r[0];
}
// what differs between the two groups in the ragged sums (k_rec_*_g2 / k_rec_*_g1)
struct RecG2 {
  using Jac = G2Jac;
  static constexpr size_t kPoint = 192, kEntry = kMsmEntryWords, kMost = 32;
  static bool tables(size_t n, size_t c, const uint8_t* p, const uint32_t* k, int32_t* t, uint8_t* cd, int nbits) {
    return job_msm_tables(n, c, p, k, t, cd, true, nbits);
  }
  static Jac ladder(size_t n, const int32_t* t, const uint8_t* cd, int nbits, MsmPart part) { return job_msm_ladder_part<true>(n, t, cd, nbits, part); }
  static void encode(const Jac& r, uint8_t* o, bool) { g2_encode_uncompressed(jac_to_affine(r), o); }  // (no paired form in G2)
};
struct RecG1 {
  using Jac = G1Jac;
  static constexpr size_t kPoint = 96, kEntry = kMsmEntryWordsG1, kMost = 64;
  static bool tables(size_t n, size_t c, const uint8_t* p, const uint32_t* k, int32_t* t, uint8_t* cd, int nbits) {
    return job_msm_tables_g1(n, c, p, k, t, cd, nbits, true);
  }
  static Jac ladder(size_t n, const int32_t* t, const uint8_t* cd, int nbits, MsmPart part) {
    return job_msm_ladder_g1_part<true>(n, t, cd, part, nbits / 2);
  }
  static void encode(const Jac& r, uint8_t* o, bool negate) {  // (the identity stays the identity: its encoding has no y)
    G1Affine a = jac_to_affine(r);
    a.y = Fq::select(negate, -a.y, a.y).norm();
    g1_encode_uncompressed(a, o);
  }
};
// launch_rec_sum_g2 / _g1 as the kernels run it: stage T chunk by chunk, stage L wave by wave (kMost / parts sums per wave,
// one trip count per wave), the parts of a sum one after the other, the `none` select, the xor tree.  points_b != null: the
// PAIRED form of launch_rec_sum_g1_pair -- 2 chunks lanes in stage T (rec_pair_chunk, rec_pair_place), the two sums of a segment
// next to each other in stage L (rec_pair_lane), A_j and -B_j interleaved in out (rec_pair_out).
template <class G>
void rec_sum(size_t J, const uint64_t* seg_first, const uint8_t* points, const uint8_t* points_b, const uint32_t* scalars, int nbits, size_t parts,
             uint8_t* out, uint8_t* status, int32_t* tbl, uint8_t* codes, const uint64_t* first_chunk) {
  const uint64_t chunks = first_chunk[J];
  if (!J || !chunks) return;
  if (parts < 1 || parts > G::kMost || (parts & (parts - 1))) parts = 1;
  const bool pair = points_b != nullptr;
  for (uint64_t t = 0; t < (pair ? rec_pair_tables_lanes(chunks) : chunks); t++) {
    const RecPairChunk h = pair ? rec_pair_chunk(t, chunks) : RecPairChunk{0, t};
    const size_t j = rec_segment_of_chunk(first_chunk, J, h.c);
    const uint64_t r0 = seg_first[j], len = seg_first[j + 1] - r0;
    const uint64_t p0 = pair ? rec_pair_place(h.half, first_chunk[j], chunks) : first_chunk[j] * kMsmChunk;
    const bool ok = G::tables((size_t)len, (size_t)(h.c - first_chunk[j]), (h.half ? points_b : points) + r0 * G::kPoint, scalars + r0 * 8,
                              tbl + p0 * 8 * G::kEntry, codes + p0 * kMsmColumns, nbits);
    if (!ok && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
  }
  const size_t per_wave = G::kMost / parts, sums = pair ? rec_pair_ladder_lanes(J, parts) / parts : J;
  for (size_t q0 = 0; q0 < sums; q0 += per_wave) {
    const size_t q1 = q0 + per_wave < sums ? q0 + per_wave : sums;
    std::vector<uint64_t> len(q1 - q0, 0), p0(q1 - q0, 0);
    std::vector<RecPairLane> who(q1 - q0);
    uint64_t trips = 0;  // (the lanes behind the last sum bring len = 0)
    for (size_t q = q0; q < q1; q++) {
      const RecPairLane w = who[q - q0] = pair ? rec_pair_lane(q * parts, parts) : RecPairLane{q, 0, 0};
      if (status[w.j] == TC_JOB_OK) {
        len[q - q0] = seg_first[w.j + 1] - seg_first[w.j];
        p0[q - q0] = !len[q - q0] ? 0 : pair ? rec_pair_place(w.half, first_chunk[w.j], chunks) : first_chunk[w.j] * kMsmChunk;
      }
      const uint64_t t = rec_part_trips(len[q - q0], parts);
      trips = t > trips ? t : trips;
    }
    for (size_t q = q0; q < q1; q++) {
      const uint64_t l = len[q - q0], p = p0[q - q0];
      const RecPairLane w = who[q - q0];
      std::vector<typename G::Jac> r(parts);
      for (size_t g = 0; g < parts; g++) {
        const RecPart rp = rec_part(l, g, parts);
        const bool none = rp.s0 >= rp.s1;
        r[g] = G::ladder(l ? (size_t)l : 1, tbl + p * 8 * G::kEntry, codes + p * kMsmColumns, nbits, MsmPart{(size_t)rp.s0, (size_t)rp.s1, (size_t)trips});
        r[g] = G::Jac::select(none, G::Jac::infinity(), r[g]);
      }
      G::encode(merge(r, parts), pair ? out + rec_pair_out(w.j, w.half) : out + w.j * G::kPoint, w.half != 0);
    }
  }
}
}  // namespace

extern "C" {
int mph_msm_g2(size_t n, size_t B, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, const uint8_t* status_in, int nbits,
               size_t parts, const uint64_t* idx, size_t n_per_job, size_t t, int need_value, uint8_t* out, uint8_t* status, int32_t* tbl,
               uint8_t* codes) {
  memcpy(status, status_in, B);
  if (need_value == 0) return 0;
  const size_t chunks = msm_chunks(n), shares4 = chunks * kMsmChunk;
  for (size_t j = 0; j < B; j++) {
    if (!taken(idx, n_per_job, t, j)) continue;
    int32_t* jt = tbl + j * shares4 * 8 * kMsmEntryWords;
    uint8_t* jc = codes + j * kMsmColumns * shares4;
    for (size_t c = 0; c < chunks; c++) {
      const bool ok = job_msm_tables(n, c, points + j * pts_stride, scalars + j * n * 8, jt, jc, true, nbits);
      if (!ok && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
    }
  }
  for (size_t j = 0; j < B; j++) {
    if (!taken(idx, n_per_job, t, j)) continue;
    if (status[j] != TC_JOB_OK) {
      g2_encode_uncompressed(G2Affine::infinity(), out + j * 192);
      continue;
    }
    const int32_t* jt = tbl + j * shares4 * 8 * kMsmEntryWords;
    const uint8_t* jc = codes + j * kMsmColumns * shares4;
    std::vector<G2Jac> r(parts);
    for (size_t g = 0; g < parts; g++)
      r[g] = parts == 1 ? job_msm_ladder(n, jt, jc, nbits) : job_msm_ladder_part<true>(n, jt, jc, nbits, msm_part(n, g, parts));
    g2_encode_uncompressed(jac_to_affine(merge(r, parts)), out + j * 192);
  }
  return 0;
}

int mph_msm_g1(size_t n, size_t B, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, const uint8_t* status_in, int nbits,
               size_t parts, uint8_t* out, uint8_t* status, int32_t* tbl, uint8_t* codes) {
  memcpy(status, status_in, B);
  const size_t chunks = msm_chunks(n), shares4 = chunks * kMsmChunk;
  const bool shared = pts_stride == 0 && nbits < 128;
  const int top = nbits / 2;
  for (size_t j = 0; j < B; j++)
    for (size_t c = 0; c < chunks; c++) {
      const bool ok = job_msm_tables_g1(n, c, points + j * pts_stride, scalars + j * n * 8, tbl + (shared ? 0 : j * shares4 * 8 * kMsmEntryWordsG1),
                                        codes + j * kMsmColumns * shares4, nbits, !shared || j == 0);
      if (!ok && status[j] == TC_JOB_OK) status[j] = TC_JOB_INVALID_ENCODING;
    }
  for (size_t j = 0; j < B; j++) {
    if (status[j] != TC_JOB_OK) {
      g1_encode_uncompressed(G1Affine::infinity(), out + j * 96);
      continue;
    }
    const int32_t* jt = tbl + (shared ? 0 : j * shares4 * 8 * kMsmEntryWordsG1);
    const uint8_t* jc = codes + j * kMsmColumns * shares4;
    std::vector<G1Jac> r(parts);
    for (size_t g = 0; g < parts; g++)
      r[g] = parts == 1 ? job_msm_ladder_g1_part<false>(n, jt, jc, msm_part(n), top) : job_msm_ladder_g1_part<true>(n, jt, jc, msm_part(n, g, parts), top);
    g1_encode_uncompressed(jac_to_affine(merge(r, parts)), out + j * 96);
  }
  return 0;
}

int mph_comb(const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, size_t share, uint8_t* out, uint8_t* status,
             uint8_t* ok, int32_t* tbl) {
  for (size_t j = 0; j < B; j++) ok[j] = job_comb_tables(pts + j * 192, (tbl_word*)(tbl + j * (size_t)kCombTableWords)) ? 1 : 0;
  const size_t chunks = (n + share - 1) / share;
  for (size_t tid = 0; tid < chunks * B; tid++) {  // chunk-major, as k_comb_sign orders its lane pairs
    const size_t c = tid / B, j = tid % B, s0 = c * share;
    const int cnt = (int)((n - s0 < share) ? n - s0 : share);
    const size_t o = j * n + s0;
    job_comb_sign(sk, N, idx + o, cnt, (const tbl_word*)(tbl + j * (size_t)kCombTableWords), ok[j] != 0, out + o * 192, status + o, true);
  }
  return 0;
}

// The G1 comb: stage T per ciphertext, stage S chunk by chunk in the lane order of k_comb_decrypt (on the host a lane's holder
// loop is its own: what the WAVE's loop adds is the device leg's to show)
int mph_comb_g1(const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, size_t share, uint8_t* out, uint8_t* status,
                uint8_t* ok, int32_t* tbl) {
  if (share < 1 || share > (size_t)kCombG1Share) return 1;
  for (size_t j = 0; j < B; j++) ok[j] = job_comb_tables_g1(pts + j * 96, tbl + j * (size_t)kCombG1TableWords) ? 1 : 0;
  const size_t chunks = (n + share - 1) / share;
  for (size_t tid = 0; tid < chunks * B; tid++) {
    const size_t c = tid / B, j = tid % B, s0 = c * share;
    const int cnt = (int)((n - s0 < share) ? n - s0 : share);
    const size_t o = j * n + s0;
    job_comb_decrypt(sk, N, idx + o, cnt, tbl + j * (size_t)kCombG1TableWords, ok[j] != 0, out + o * 96, status + o);
  }
  return 0;
}

// The ragged sums: J segments of one record array (seg_first: J + 1 values), out (J x 96 / 192 and whatever the caller keeps behind
// them), status (J), tbl / codes (the launch's chunks and whatever the caller keeps behind them), first_chunk (J + 1, written).
int mph_rec_sum(int w, size_t J, const uint64_t* seg_first, const uint8_t* points, const uint32_t* scalars, const uint8_t* status_in, int nbits,
                size_t parts, uint8_t* out, uint8_t* status, int32_t* tbl, uint8_t* codes, uint64_t* first_chunk) {
  memcpy(status, status_in, J);
  rec_chunk_ranges(seg_first, J, first_chunk);
  if (w == 2) rec_sum<RecG2>(J, seg_first, points, nullptr, scalars, nbits, parts, out, status, tbl, codes, first_chunk);
  else rec_sum<RecG1>(J, seg_first, points, nullptr, scalars, nbits, parts, out, status, tbl, codes, first_chunk);
  return 0;
}
// The paired sums: out (2 J x 96), tbl / codes (2 x the launch's chunks), each with whatever the caller keeps behind them
int mph_rec_sum_pair(size_t J, const uint64_t* seg_first, const uint8_t* points_a, const uint8_t* points_b, const uint32_t* scalars,
                     const uint8_t* status_in, int nbits, size_t parts, uint8_t* out, uint8_t* status, int32_t* tbl, uint8_t* codes, uint64_t* first_chunk) {
  memcpy(status, status_in, J);
  rec_chunk_ranges(seg_first, J, first_chunk);
  rec_sum<RecG1>(J, seg_first, points_a, points_b, scalars, nbits, parts, out, status, tbl, codes, first_chunk);
  return 0;
}
// k_rec_gather_keys: keys (R x 96 and whatever the caller keeps behind them)
int mph_rec_gather_keys(const uint8_t* pks, size_t K, const uint64_t* key_idx, size_t R, uint8_t* keys) {
  for (size_t r = 0; r < R; r++) {
    if (key_idx[r] < K) memcpy(keys + r * 96, pks + (size_t)key_idx[r] * 96, 96);
    else memset(keys + r * 96, 0xff, 96);
  }
  return 0;
}
void mph_rec_part(uint64_t len, size_t g, size_t parts, uint64_t* out3) {
  const RecPart p = rec_part(len, g, parts);
  out3[0] = p.s0;
  out3[1] = p.s1;
  out3[2] = rec_part_trips(len, parts);
}
// out3: table bytes in G2, in G1, code bytes of a launch of `chunks` chunks (k_msm.hip rec_table_bytes / rec_code_bytes)
void mph_rec_sizes(uint64_t chunks, size_t* out3) {
  out3[0] = (size_t)chunks * kMsmChunk * 8 * kMsmEntryWords * sizeof(int32_t);
  out3[1] = (size_t)chunks * kMsmChunk * 8 * kMsmEntryWordsG1 * sizeof(int32_t);
  out3[2] = (size_t)chunks * kMsmChunk * kMsmColumns;
}
void mph_msm_part(size_t n, size_t g, size_t parts, size_t* out3) {
  const MsmPart p = msm_part(n, g, parts);
  out3[0] = p.s0;
  out3[1] = p.s1;
  out3[2] = p.trips;
}
void mph_sizes(size_t n, size_t B, size_t* out4) {
  out4[0] = B * msm_chunks(n) * kMsmChunk * 8 * kMsmEntryWords * sizeof(int32_t);
  out4[1] = B * kMsmColumns * msm_chunks(n) * kMsmChunk;
  out4[2] = B * msm_chunks(n) * kMsmChunk * 8 * kMsmEntryWordsG1 * sizeof(int32_t);
  out4[3] = B * (size_t)kCombTableWords * sizeof(int32_t);
}
}

// ---- blame by bisection (k_blame.hip; tc_blame_jobs.h): the entries of tests/device/manypoint_blame.hip ----
namespace {
void key_words(const uint8_t* b, uint32_t* w) {
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
// k_blame_seed, then k_blame_leaves leaf by leaf (every lane is its own leader)
template <class F>
void blame_leaves(const uint8_t* key32, uint64_t call, uint64_t leaf0, const uint8_t* pts, size_t period, uint8_t* live, size_t n, uint8_t* seed_out,
                  int32_t* leaves) {
  uint32_t key[8], seed[8];
  key_words(key32, key);
  blame_call_seed(key, call, seed);
  for (int w = 0; w < 8; w++)
    for (int b = 0; b < 4; b++) seed_out[4 * w + b] = (uint8_t)(seed[w] >> (8 * b));
  key_words(seed_out, key);  // (k_blame_leaves reads the seed's bytes)
  for (size_t r = 0; r < n; r++)
    job_blame_leaf<F>(key, leaf0 + r, pts + (period ? r % period : r) * PointIO<F>::BYTES, live ? live + r : nullptr, true, leaves + r * BlameLeaf<F>::WORDS);
}
// launch_blame_range_sum's normalisation, then k_blame_range_sum item by item: the parts one after the other, the xor tree, one
// conversion.  (On the host a lane is a wave: the masked trips of job_blame_range_part are the device leg's to execute.)
template <class F>
void blame_sums(const int32_t* leaves, size_t N, const uint32_t* job, const uint32_t* lo, const uint32_t* hi, size_t n_items, size_t parts, uint8_t* out) {
  const size_t most = std::is_same<F, Fq2>::value ? 32 : 64;
  if (parts < 1 || parts > most || (parts & (parts - 1))) parts = 1;
  for (size_t it = 0; it < n_items; it++) {
    std::vector<Jac<F>> r(parts);
    for (size_t g = 0; g < parts; g++) r[g] = job_blame_range_part<F>(leaves + (size_t)job[it] * N * BlameLeaf<F>::WORDS, lo[it], hi[it], g, parts);
    PointIO<F>::encode(jac_to_affine(merge(r, parts)), out + it * PointIO<F>::BYTES);
  }
}
template <class F>
void blame_ladder(const uint8_t* pts, const uint8_t* live, const uint64_t* digits, size_t n, int32_t* leaves) {
  for (size_t r = 0; r < n; r++) {
    Affine<F> p = Affine<F>::infinity();
    const bool ok = PointIO<F>::decode(pts + r * PointIO<F>::BYTES, p) && live[r] != 0;
    if constexpr (std::is_same<F, Fq2>::value) blame_store_leaf(leaves + r * BlameLeaf<F>::WORDS, blame_leaf_g2(p, ok, digits + 4 * r));
    else blame_store_leaf(leaves + r * BlameLeaf<F>::WORDS, blame_leaf_g1(p, ok, digits + 4 * r));
  }
}
}  // namespace

extern "C" {
// leaves: n rows, live_out: n bytes (copied from live_in first), each with whatever the caller keeps behind them
int mph_blame_leaves(int g2, const uint8_t* key32, uint64_t call, uint64_t leaf0, const uint8_t* pts, size_t n_pts, size_t period,
                     const uint8_t* live_in, size_t n, uint8_t* seed_out, int32_t* leaves, uint8_t* live_out) {
  if (!n || n_pts != (period ? period : n)) return 1;
  if (live_in) memcpy(live_out, live_in, n);
  if (g2) blame_leaves<Fq2>(key32, call, leaf0, pts, period, live_in ? live_out : nullptr, n, seed_out, leaves);
  else blame_leaves<Fq>(key32, call, leaf0, pts, period, live_in ? live_out : nullptr, n, seed_out, leaves);
  return 0;
}
int mph_blame_range_sum(int g2, const int32_t* leaves, size_t F, size_t N, const uint32_t* job, const uint32_t* lo, const uint32_t* hi, size_t n_items,
                        size_t parts, uint8_t* out) {
  for (size_t i = 0; i < n_items; i++)
    if (job[i] >= F || lo[i] >= hi[i] || hi[i] > N) return 1;  // (an empty range is outside the kernel's contract)
  if (g2) blame_sums<Fq2>(leaves, N, job, lo, hi, n_items, parts, out);
  else blame_sums<Fq>(leaves, N, job, lo, hi, n_items, parts, out);
  return 0;
}
int mph_blame_chain(int g2, const uint8_t* key32, uint64_t call, uint64_t leaf0, const uint8_t* pts, size_t n_pts, size_t period, const uint8_t* live_in,
                    size_t n, const uint32_t* lo, const uint32_t* hi, size_t n_items, size_t parts, uint8_t* seed_out, uint8_t* live_out, uint8_t* out) {
  std::vector<int32_t> leaves(n * (size_t)(g2 ? kBlameLeafWordsG2 : kBlameLeafWordsG1));
  std::vector<uint32_t> job(n_items, 0);
  const int rc = mph_blame_leaves(g2, key32, call, leaf0, pts, n_pts, period, live_in, n, seed_out, leaves.data(), live_out);
  return rc ? rc : mph_blame_range_sum(g2, leaves.data(), 1, n, job.data(), lo, hi, n_items, parts, out);
}
int mph_blame_ladder(int g2, const uint8_t* pts, const uint8_t* live, const uint64_t* digits, size_t n, int32_t* leaves) {
  if (g2) blame_ladder<Fq2>(pts, live, digits, n, leaves);
  else blame_ladder<Fq>(pts, live, digits, n, leaves);
  return 0;
}
size_t mph_blame_leaf_bytes(int g2) { return (size_t)(g2 ? kBlameLeafWordsG2 : kBlameLeafWordsG1) * sizeof(int32_t); }
}

#if defined(MP_MAIN)
#include "../../threshold_crypto_amd/csrc/tc_dkg.h"  // g1_mul_u64, for the inputs
static void fr_words(uint64_t lo, uint32_t* w) {
  memset(w, 0, 32);
  w[0] = (uint32_t)lo;
  w[1] = (uint32_t)(lo >> 32);
}
int main() {
  int rc = 0;
  const size_t n = 9, B = 2;
  size_t sz[4];
  mph_sizes(n, B, sz);
  // G1: k g1 for k = 2 .. ; share 3 of job 0 the identity, shares 0 and 1 of job 1 equal with equal scalars
  std::vector<uint8_t> p1(B * n * 96), st0(B, 0), st(B), out(B * 96), out1(B * 96), codes(sz[1]);
  std::vector<uint32_t> sc(B * n * 8);
  for (size_t i = 0; i < B * n; i++) {
    g1_encode_uncompressed(jac_to_affine(g1_mul_u64(G1Jac::from_affine(g1_generator()), i == n + 1 ? n + 2 : i + 2)), p1.data() + i * 96);
    fr_words(i == n + 1 ? 0x1234567 : 0x1234567 + 2 * i * i, sc.data() + i * 8);
  }
  memset(p1.data() + 3 * 96, 0, 96);
  p1[3 * 96] = 0x40;
  std::vector<int32_t> t1(sz[2] / 4);
  for (size_t parts = 1; parts <= 2; parts *= 2) {
    rc |= mph_msm_g1(n, B, n * 96, p1.data(), sc.data(), st0.data(), 128, parts, parts == 1 ? out1.data() : out.data(), st.data(), t1.data(), codes.data());
    rc |= st[0] | st[1];
    if (parts > 1) rc |= memcmp(out.data(), out1.data(), out.size()) ? 1 : 0;
  }
  // short scalars over the shared set: the same sum as over own points (job 0's)
  for (size_t i = 0; i < B * n; i++) fr_words(2 * i + 1, sc.data() + i * 8);
  rc |= mph_msm_g1(n, 1, n * 96, p1.data(), sc.data(), st0.data(), 32, 2, out1.data(), st.data(), t1.data(), codes.data());
  rc |= mph_msm_g1(n, B, 0, p1.data(), sc.data(), st0.data(), 32, 1, out.data(), st.data(), t1.data(), codes.data());
  rc |= st[0] | st[1] | (memcmp(out.data(), out1.data(), 96) ? 1 : 0);
  // G2: the points come from the comb signer: sk[i] g2 for the keys 1 .. 9
  std::vector<uint8_t> sk(n * 32, 0), h(192), shares(n * 192), sst(n), okb(1), o2(B * 192), o21(B * 192);
  for (size_t i = 0; i < n; i++) sk[i * 32] = (uint8_t)(i + 1);  // little-endian Fr: keys 1 .. 9
  g2_encode_uncompressed(G2Affine{Fq2::make(Fq::from_mont384(G2_GEN_X0), Fq::from_mont384(G2_GEN_X1)),
                                  Fq2::make(Fq::from_mont384(G2_GEN_Y0), Fq::from_mont384(G2_GEN_Y1)), false},
                         h.data());
  std::vector<uint64_t> idx(n);
  for (size_t i = 0; i < n; i++) idx[i] = i;
  std::vector<int32_t> ct(sz[3] / 4 / B);
  for (size_t share = 1; share <= 8; share += 3) {
    rc |= mph_comb(sk.data(), n, idx.data(), h.data(), n, 1, share, shares.data(), sst.data(), okb.data(), ct.data());
    for (size_t i = 0; i < n; i++) rc |= sst[i];
    rc |= okb[0] == 1 ? 0 : 1;
  }
  rc |= memcmp(shares.data(), h.data(), 192) ? 1 : 0;  // key 1
  std::vector<uint8_t> p2(B * n * 192);
  for (size_t i = 0; i < B * n; i++) memcpy(p2.data() + i * 192, shares.data() + (i % n) * 192, 192);
  memset(p2.data() + 4 * 192, 0, 192);
  p2[4 * 192] = 0x40;
  for (size_t i = 0; i < B * n; i++) fr_words(0xabcdef01 + 2 * i * i * i, sc.data() + i * 8);
  std::vector<int32_t> t2(sz[0] / 4);
  for (size_t parts = 1; parts <= 2; parts *= 2) {
    rc |= mph_msm_g2(n, B, n * 192, p2.data(), sc.data(), st0.data(), 64, parts, nullptr, 0, 0, -1, parts == 1 ? o21.data() : o2.data(), st.data(), t2.data(),
                     codes.data());
    rc |= st[0] | st[1];
    if (parts > 1) rc |= memcmp(o2.data(), o21.data(), o2.size()) ? 1 : 0;
  }
  for (size_t i = 0; i < B * n; i++) fr_words(2 * i + 1, sc.data() + i * 8);
  rc |= mph_msm_g2(n, B, n * 192, p2.data(), sc.data(), st0.data(), 16, 2, nullptr, 0, 0, -1, o2.data(), st.data(), t2.data(), codes.data());
  rc |= st[0] | st[1];
  sc[0] = 2;  // an even short scalar fails its job
  rc |= mph_msm_g2(n, B, n * 192, p2.data(), sc.data(), st0.data(), 16, 1, nullptr, 0, 0, -1, o2.data(), st.data(), t2.data(), codes.data());
  rc |= (st[0] == TC_JOB_INVALID_ENCODING && st[1] == TC_JOB_OK && o2[0] == 0x40) ? 0 : 1;
  // ragged sums, one case per group: segments of 0, 1, 5, 0, 2 and 3 records over the points and (short, odd) scalars above;
  // every split gives the bytes of parts = 1, empty segments give the identity, [1] P = P
  {
    const uint64_t seg[7] = {0, 0, 1, 6, 6, 8, 11};
    const size_t J = 6;
    std::vector<uint64_t> fc(J + 1);
    std::vector<uint8_t> st6(J), z6(J, 0);
    for (size_t i = 0; i < B * n; i++) fr_words(2 * i + 1, sc.data() + i * 8);
    for (int w = 1; w <= 2; w++) {
      const size_t pt = w == 2 ? 192 : 96;
      const uint64_t C = 5;  // 0 + 1 + 2 + 0 + 1 + 1 chunks, and one more behind them that must stay as it is
      size_t rs[3];
      mph_rec_sizes(C + 1, rs);
      std::vector<int32_t> tb(rs[w == 2 ? 0 : 1] / 4);
      std::vector<uint8_t> cd(rs[2]), ro(J * pt), ro1(J * pt);
      const uint8_t* pp = w == 2 ? p2.data() : p1.data();
      for (size_t parts : {(size_t)1, (size_t)2, (size_t)8, (size_t)32, (size_t)3}) {
        std::fill(tb.begin(), tb.end(), 0x5A5A5A5A);
        std::fill(cd.begin(), cd.end(), (uint8_t)0x5A);
        rc |= mph_rec_sum(w, J, seg, pp, sc.data(), z6.data(), w == 2 ? 16 : 32, parts, parts == 1 ? ro1.data() : ro.data(), st6.data(), tb.data(),
                          cd.data(), fc.data());
        for (size_t j = 0; j < J; j++) rc |= st6[j];
        rc |= fc[J] == C ? 0 : 1;
        if (parts != 1) rc |= memcmp(ro.data(), ro1.data(), ro.size()) ? 1 : 0;
        for (size_t i = tb.size() / (C + 1) * C; i < tb.size(); i++) rc |= tb[i] == 0x5A5A5A5A ? 0 : 1;
        for (size_t i = cd.size() / (C + 1) * C; i < cd.size(); i++) rc |= cd[i] == 0x5A ? 0 : 1;
      }
      rc |= (ro1[0] == 0x40 && ro1[3 * pt] == 0x40) ? 0 : 1;
      rc |= memcmp(ro1.data() + pt, pp, pt) ? 1 : 0;  // (record 0 has the scalar 1)
    }
    // the paired sums over the same segments: a = the G1 points, b = the same array from record 3 on (b's first record is the
    // identity); half 0 is the unpaired sum over a, half 1 has the x of the unpaired sum over b, every split gives the same bytes
    {
      const uint64_t C = 5;
      size_t rs[3];
      mph_rec_sizes(2 * C + 1, rs);
      std::vector<int32_t> tb(rs[1] / 4);
      std::vector<uint8_t> cd(rs[2]), ua(J * 96), ub(J * 96), po(2 * J * 96), po1(2 * J * 96);
      const uint8_t* pb = p1.data() + 3 * 96;
      rc |= mph_rec_sum(1, J, seg, p1.data(), sc.data(), z6.data(), 32, 1, ua.data(), st6.data(), tb.data(), cd.data(), fc.data());
      rc |= mph_rec_sum(1, J, seg, pb, sc.data(), z6.data(), 32, 1, ub.data(), st6.data(), tb.data(), cd.data(), fc.data());
      for (size_t parts : {(size_t)1, (size_t)2, (size_t)16, (size_t)64, (size_t)3}) {
        std::fill(tb.begin(), tb.end(), 0x5A5A5A5A);
        std::fill(cd.begin(), cd.end(), (uint8_t)0x5A);
        rc |= mph_rec_sum_pair(J, seg, p1.data(), pb, sc.data(), z6.data(), 32, parts, parts == 1 ? po1.data() : po.data(), st6.data(), tb.data(),
                               cd.data(), fc.data());
        for (size_t j = 0; j < J; j++) rc |= st6[j];
        if (parts != 1) rc |= memcmp(po.data(), po1.data(), po.size()) ? 1 : 0;
        for (size_t i = tb.size() / (2 * C + 1) * 2 * C; i < tb.size(); i++) rc |= tb[i] == 0x5A5A5A5A ? 0 : 1;
        for (size_t i = cd.size() / (2 * C + 1) * 2 * C; i < cd.size(); i++) rc |= cd[i] == 0x5A ? 0 : 1;
        rc |= memcmp(cd.data(), cd.data() + C * kMsmChunk * kMsmColumns, C * kMsmChunk * kMsmColumns) ? 1 : 0;  // the same scalars
      }
      for (size_t j = 0; j < J; j++) {
        rc |= memcmp(po1.data() + 2 * j * 96, ua.data() + j * 96, 96) ? 1 : 0;
        rc |= memcmp(po1.data() + (2 * j + 1) * 96, ub.data() + j * 96, 48) ? 1 : 0;
        const bool inf = ub[j * 96] == 0x40;  // -B_j: the identity as it is, else another y
        rc |= (memcmp(po1.data() + (2 * j + 1) * 96 + 48, ub.data() + j * 96 + 48, 48) == 0) == inf ? 0 : 1;
      }
    }
    // the G1 comb: the keys 1 .. 9 over u = 2 g1 and over the identity, at 1, 4 and 8 holders per lane
    {
      const size_t Bc = 2;
      std::vector<uint8_t> u(Bc * 96), co(Bc * n * 96), co1(Bc * n * 96), cs(Bc * n), cok(Bc);
      memcpy(u.data(), p1.data(), 96);
      memcpy(u.data() + 96, p1.data() + 3 * 96, 96);
      std::vector<uint64_t> ci(Bc * n);
      for (size_t i = 0; i < Bc * n; i++) ci[i] = i % n;
      std::vector<int32_t> ct1(Bc * (size_t)kCombG1TableWords);
      for (size_t share : {(size_t)1, (size_t)4, (size_t)8}) {
        rc |= mph_comb_g1(sk.data(), n, ci.data(), u.data(), n, Bc, share, share == 1 ? co1.data() : co.data(), cs.data(), cok.data(), ct1.data());
        for (size_t i = 0; i < Bc * n; i++) rc |= cs[i];
        rc |= (cok[0] == 1 && cok[1] == 1) ? 0 : 1;
        if (share != 1) rc |= memcmp(co.data(), co1.data(), co.size()) ? 1 : 0;
      }
      rc |= memcmp(co1.data(), u.data(), 96) ? 1 : 0;             // key 1
      rc |= memcmp(co1.data() + 96, p1.data() + 2 * 96, 96) ? 1 : 0;  // key 2 over 2 g1: record 2 is 4 g1
      for (size_t i = 0; i < n; i++) rc |= co1[(n + i) * 96] == 0x40 ? 0 : 1;
    }
    uint8_t keys[3 * 96 + 96];
    memset(keys, 0x5A, sizeof keys);
    const uint64_t ki[3] = {1, 2, ~0ull};
    rc |= mph_rec_gather_keys(p1.data(), 2, ki, 3, keys);
    rc |= (memcmp(keys, p1.data() + 96, 96) == 0 && keys[96] == 0xff && keys[3 * 96 - 1] == 0xff && keys[3 * 96] == 0x5A) ? 0 : 1;
  }
  printf("manypoint_host: %s\n", rc ? "FAILED" : "ok");
  return rc ? 1 : 0;
}
#endif
