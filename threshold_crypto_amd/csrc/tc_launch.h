// Host-side launch prototypes of the gfx950 kernels (one translation unit per kernel family
// so hipcc can build them in parallel).  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "tc_arena.h"

namespace tc {

// waves per SIMD the register allocator must leave room for (__launch_bounds__ 2nd argument).
// Kernels on Fq2 values run two lanes per job (tc_common.h): batch 65 536 gives them two waves
// per SIMD, so they are compiled for 256 registers; the G1 kernels keep the full 512.
#ifndef TC_WAVES_G2
#define TC_WAVES_G2 2
#endif
#ifndef TC_WAVES_G1
#define TC_WAVES_G1 1
#endif
// the G1 kernels of the paths beside the headline (Commitment::evaluate, BivarCommitment::row, the general-path combination and
// small linear combinations): built for 256 registers.  One lane per job gives a 65 536-job batch one wave per SIMD whatever the
// build, and from 131 072 jobs on the second wave is worth 4-15 % although 100-250 registers spill (r04: profiles/r04_g1_aux_probe.txt)
#ifndef TC_WAVES_G1_AUX
#define TC_WAVES_G1_AUX 2
#endif
constexpr int kBlock = 64;  // one wavefront per workgroup: the jobs are register/scratch heavy

inline unsigned grid_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// Two jobs per lane pair (tc_duo.h: checked G2 decodes, hash_g2, hash_g1_g2) halves the lanes of a launch and lengthens each: it
// pays once the launch is large enough that the halved form still fills the SIMDs.  Measured (profiles/r05_duo_sweep.txt, one
// MI355X, ms one job per pair / two):
//   decode   32 768: 2.03 / 2.47    65 536: 3.29 / 2.68   131 072: 6.72 / 4.57   262 144: 12.90 / 9.43
//   hash_g2  32 768: 5.13 / 8.58    65 536: 8.27 / 9.02   131 072: 15.56 / 14.42 262 144: 30.43 / 27.47
// A third of a decode is Fq-only work (two exponentiations), so it wins as soon as the one-job form needs a second wave on any
// SIMD (more than 32 768 points); a hash has 24 % of it and a search loop that runs until the slowest of 64 instead of 32
// messages has its candidate, so it only wins with two waves per SIMD in the halved form (131 072 messages).
constexpr size_t kDuoMinDecode = 32768 + 1;
constexpr size_t kDuoMinHash = 131072;
inline bool duo_form(size_t jobs, size_t min_jobs) { return jobs >= min_jobs; }

// Decryption shares of many holders per ciphertext (tc_decrypt_shares_g1_batch): the per-ciphertext G1 comb (k_comb.hip) from this
// many holders and this many ciphertexts on, one arena ladder per share below.  Measured (profiles/decrypt_shares_probe.txt, one
// MI355X, ms comb / ladders): a comb is built by ONE lane per ciphertext in 128 dependent doubling steps, ~17 ms whatever the batch,
// and a share then costs 0.4-0.5 of a ladder --
//   n = 68:      B = 1 024: 17.7 / 3.8    4 096: 20.9 / 9.9    16 384: 31.8 / 30.9    65 536: 74.8 / 117.5    131 072: 125.4 / 234.0
//   B = 65 536:  n = 4: 23.4 / 7.6    8: 26.1 / 14.7    16: 32.4 / 28.7    32: 51.0 / 56.0;      B = 131 072, n = 16: 53.7 / 56.1
// -- so it pays from about 1.3 million shares per call on.  The two thresholds keep every call they admit above that.
constexpr size_t kCombG1MinHolders = 24;
constexpr size_t kCombG1MinBatch = 65536;

// The form choices of a context.  The defaults are the measured thresholds above / in k_pairing.hip; the environment
// (TC_DUO_MIN=<jobs>, TC_PAIRING_FORM=quad|lines|pair|fused, TC_PAIRING_BUDGET=<bytes>, TC_CHECKS_BESIDE=0|1: tests and experiments) is read ONCE,
// when the context is created (tc_api.hip tuning_from_env) -- no getenv on the launch path, nothing a concurrent setenv can race
// with -- and tc_ctx_get_tuning reports what a context uses.
constexpr size_t kMaxPrivateBytesPerLane = 12288;  // >= the largest private segment of any kernel (11 152 B: k_rec_tables_g1; tests/test_abi.py)
struct Tuning {
  size_t duo_min_decode = kDuoMinDecode, duo_min_hash = kDuoMinHash;
  int pairing_form = 0;       // 0 = by batch size; 1 quad, 2 lines (prepared), 3 pair (one loop), 4 fused
  size_t pairing_budget = 0;  // bytes the prepared form's line buffer may take; 0 = a third of the HBM that is free
  // free HBM a call insists on before it launches (after its own allocations): the ROCm runtime allocates the kernels' private
  // segments (scratch) at dispatch and ABORTS THE PROCESS when it cannot (amd::roc::callbackQueue <- AqlQueue::DynamicQueueEventsHandler,
  // seen with ~0.4 GB free).  (size_t)-1 = by the size of the call (Call::guard_private); TC_PRIVATE_RESERVE=<bytes> fixes it, 0 disables.
  size_t private_reserve = (size_t)-1;
  size_t msm_budget = 0;      // bytes the per-share tables of the two-stage kernels may take per call; 0 = a third of the free HBM, 1-24 GiB (TC_MSM_BUDGET: tests)
  int checks_beside = 1;  // checked-input mode: the membership tests on a second stream beside the call's main kernels (TC_CHECKS_BESIDE=0: before them, one stream)
  size_t sum_parts = 0;   // lanes per output of k_g1_sum (TC_SUM_PARTS=<1|2|4|...|64>: tests, tools/g1_sum_probe.py); 0 = by B, n and the CU count (g1_sum_parts)
  size_t wsum_slices = 0; // slices per output of k_g1_wsum (TC_WSUM_SLICES=<n>: tests, tools/dkg_reshare_probe.py); 0 = by B, n and the CU count (g1_wsum_slices)
  size_t records_parts = 0;  // lanes / lane pairs per segment of the ragged sums (TC_RECORDS_PARTS=<1|2|...|64>: tests, tools/verify_records_probe.py); 0 = rec_parts
  // tc_decrypt_shares_*: the G1 comb from this many holders AND this many ciphertexts on (TC_COMB_G1_MIN="<holders>,<batch>": tests,
  // tools/decrypt_shares_probe.py)
  size_t comb_g1_min_holders = kCombG1MinHolders, comb_g1_min_batch = kCombG1MinBatch;
  // the resident waves the launch order of the grouped G2 combination folds at (TC_COMBINE_SEATS=<waves>: tests); 0 = the device's own
  // (k_combine.hip combine_g2_seats)
  uint32_t combine_seats = 0;
};

// The G1 ladder kernels keep their per-lane table in the HBM arena and fit 256 registers (two waves per SIMD) at
// EVERY batch size since the end of r04: the register-table builds they replaced (377 registers + 121 AGPRs, 7 KB of scratch per
// lane) were no faster below 65 536 jobs (profiles/r04_g1_arena_all_sizes.txt: single multiplications 7-16 % SLOWER, the
// combination 1 % faster) and are only compiled with -DTC_G1_ARENA_MIN=<jobs> (experiments).
#ifndef TC_G1_ARENA_MIN
#define TC_G1_ARENA_MIN 0
#endif
constexpr size_t kG1ArenaMinJobs = TC_G1_ARENA_MIN;
void launch_g1_mul(hipStream_t st, TableArena ta, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, uint8_t* out,
                   uint8_t* status);
void launch_g2_mul(hipStream_t st, TableArena ta, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, uint8_t* out,
                   uint8_t* status);
// out[j*n + k] = sk[idx[j*n + k]] * pts[j]: the shares of message j by its n selected signers out of N
void launch_g2_mul_gather(hipStream_t st, TableArena ta, const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B,
                          uint8_t* out, uint8_t* status);
// many signers per message (n >= kCombMinSigners): a per-message comb in HBM (tbl: comb_table_bytes(B), ok: B bytes), then
// doubling-free multiplications (k_comb.hip)
constexpr size_t kCombMinSigners = 24;
// ... and enough messages: a comb is built by ONE lane pair per message in 64 dependent column steps (~15 ms whatever the
// batch), which only pays from a few thousand messages on; below, the per-chunk ladders of k_g2_mul_gather
constexpr size_t kCombMinBatch = 8192;
// signers a lane pair of the share-generation kernels takes: `most` (one table / one inversion shared by eight) when the
// batch fills the GPU that way; for a smaller batch the smallest number that keeps the launch within ONE round of the
// 2048 wave slots (65 536 lane pairs) -- more, shorter lane pairs, no second round with a handful of waves
inline size_t signers_per_lane_pair(size_t n, size_t B, size_t most) {
  for (size_t share = 1; share < most; share++)
    if (((n + share - 1) / share) * B <= 65536) return share;
  return most;
}
size_t comb_table_bytes(size_t B);
void launch_comb_sign(hipStream_t st, TableArena ta, const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B,
                      int32_t* tbl, uint8_t* ok, uint8_t* out, uint8_t* status);
// The same for decryption shares (k_comb.hip, tc_comb_g1.h): out[j*n + k] = sk[idx[j*n + k]] * pts[j] in G1, the shares of
// ciphertext j by its n selected key holders out of N.  launch_comb_decrypt: a per-ciphertext comb in HBM (tbl:
// comb_table_bytes_g1(B), ok: B bytes), then doubling-free multiplications; launch_g1_mul_gather: one arena ladder per share.
// The comb runs from kCombG1MinHolders holders and kCombG1MinBatch ciphertexts on (TC_COMB_G1_MIN="<holders>,<batch>" at
// context creation overrides both: Tuning::comb_g1_min_*, above).
// holders a lane of k_comb_decrypt takes: the G1 twin of signers_per_lane_pair -- one lane per job, so ONE round of the 2048
// wave slots is 131 072 lanes
inline size_t holders_per_lane(size_t n, size_t B, size_t most) {
  for (size_t share = 1; share < most; share++)
    if (((n + share - 1) / share) * B <= 131072) return share;
  return most;
}
size_t comb_table_bytes_g1(size_t B);
void launch_comb_decrypt(hipStream_t st, const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, int32_t* tbl,
                         uint8_t* ok, uint8_t* out, uint8_t* status);
void launch_g1_mul_gather(hipStream_t st, TableArena ta, const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B,
                          uint8_t* out, uint8_t* status);
void launch_g1_compress(hipStream_t st, const uint8_t* in, size_t B, uint8_t* out, uint8_t* status);
void launch_g2_compress(hipStream_t st, const uint8_t* in, size_t B, uint8_t* out, uint8_t* status);
void launch_g1_decompress(hipStream_t st, const uint8_t* in, size_t B, uint8_t* out, uint8_t* status);
void launch_g2_decompress(const Tuning& tn, hipStream_t st, const uint8_t* in, size_t B, uint8_t* out, uint8_t* status);
// wire ingest of the combiners: the first `take` of n_per_job compressed samples per job, checked decode, compact output
// (B x take points) + one validity byte per sample; and the matching prefix of the index array
void launch_decompress_take(const Tuning& tn, hipStream_t st, bool g2, const uint8_t* in, size_t n_per_job, size_t take, size_t B, uint8_t* out, uint8_t* valid);
void launch_take_u64(hipStream_t st, const uint64_t* in, size_t n_per_job, size_t take, size_t B, uint64_t* out);

// need_general: one zeroed device word; the Lagrange stage counts the jobs the small-index fast path
// does not take, the general combine kernel leaves at once when it stays zero (k_combine.hip).  counted: the word holds
// that count already (launch_combine_g2's grouping made it): nothing is added, and zero ends the kernel at once
void launch_lagrange(hipStream_t st, const uint64_t* idx, size_t n_per_job, size_t t, size_t B, uint32_t* lam,
                     uint8_t* status, uint32_t* need_general, bool counted = false);
// every coefficient of a job from ONE lane with one inversion (large thresholds); ws: lagrange_all_ws_words
size_t lagrange_all_ws_words(size_t t, size_t B);
void launch_lagrange_all(hipStream_t st, const uint64_t* idx, size_t n_per_job, size_t t, size_t B, uint32_t* lam, uint32_t* ws,
                         uint8_t* status);
// ta: the table arena (the fast path's per-lane ladder tables); may be empty when idx == nullptr (no fast path)
// cls / counters / perm (all three or none): scratch of the caller for grouping the fast path's jobs by denominator class, as in G2
void launch_combine_g1(hipStream_t st, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares,
                       const uint32_t* lam, size_t B, uint8_t* out, uint8_t* status, const uint32_t* need_general,
                       TableArena ta = TableArena{nullptr, nullptr}, uint8_t* cls = nullptr, uint32_t* counters = nullptr,
                       uint32_t* perm = nullptr, hipEvent_t before_main = nullptr);
// From this many jobs on the G1 fast path groups its jobs by denominator class (a wave of D = 1 jobs -- a fifth of the 4-of-10
// subsets -- skips the [1 / D] ladder).  It only pays once a SIMD sees several rounds of waves: measured 3.5 % slower at 131 072
// jobs (every wave resident at once: the launch lasts as long as two generic waves on one SIMD, grouped or not), equal at
// 262 144, 8 % faster at 524 288 (profiles/r04_g1_group_ab.txt).
constexpr size_t kG1GroupMinJobs = 524288;
// `T: IntoFr` abscissae beyond u64 (tc_combine_g{1,2}_fr_batch): idx_fr = B x n_per_job x 8 canonical LE words.
//   launch_fr_idx_narrow   idx64[i] = the value when it fits 64 bits; *wide counts the ones that do not; valid[j] (preset
//                          to 1) is cleared for a job that owns a non-canonical encoding (>= r) among its first `take`
//   launch_lagrange_fr     lambda_i of every job from the Fr abscissae x = idx_fr + 1 (one lane per coefficient)
void launch_fr_idx_narrow(hipStream_t st, const uint32_t* idx_fr, size_t n_per_job, size_t take, size_t B, uint64_t* idx64, uint32_t* wide,
                          uint8_t* valid);
void launch_lagrange_fr(hipStream_t st, const uint32_t* idx_fr, size_t n_per_job, size_t t, size_t B, uint32_t* lam, uint8_t* status);
size_t combine_group_slots(size_t B);
// G2 groups its fast-path jobs by index tuple (k_combine.hip): gws = combine_group_ws_words(B) words and perm =
// combine_group_slots_g2(B) words of the caller's scratch, both or neither.  With both the launch also counts the jobs the
// fast path leaves, in the word combine_group_need(gws) of the workspace, and launches the call's Lagrange stage itself
// (launch_lagrange, counted) -- the caller launches none and hands that word to what runs behind (MsmFilter::need)
size_t combine_group_slots_g2(size_t B);
size_t combine_group_ws_words(size_t B);
uint32_t* combine_group_need(uint32_t* gws);
void launch_combine_g2(hipStream_t st, TableArena ta, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares,
                       uint32_t* lam, size_t B, uint8_t* out, uint8_t* status, uint32_t* gws,
                       uint32_t* perm, const uint32_t* need_general, hipEvent_t before_main = nullptr);
// The launch order of that grouping folds at the waves of k_combine_fast<Fq2> the device holds at once: CUs x occupancy, which
// launch_combine_g2 asks the runtime for once per device.  A context created under TC_COMBINE_SEATS=<waves> (Tuning::combine_seats;
// tests: a "device" of 64 or 128 seats) puts its value here, for the calling thread, just before it launches; the launcher takes
// it and clears it, so nothing set for one call reaches another; 0 = the device's own.  (A variable and not a parameter: the
// launcher's signature is what the host harness of the call frame, tests/call, links its stand-ins against.)
inline thread_local uint32_t t_combine_seats = 0;
// shared_points: every job combines the SAME n points (points holds n of them) with its own n scalars
void launch_lincomb_g1(hipStream_t st, size_t n, const uint8_t* scalars, const uint8_t* points, size_t B, uint8_t* out,
                       uint8_t* status, bool shared_points = false);
// random-linear-combination share validation (k_check.hip): 64-bit scalars from a ChaCha20 stream keyed
// by the caller's seed; row gather / byte scatter for the per-share fallback of failed messages
void launch_rlc_scalars(hipStream_t st, const uint8_t* seed32, size_t n, uint8_t* out_fr);
void launch_gather_rows(hipStream_t st, const uint8_t* src, size_t row_bytes, const uint32_t* map, size_t rows, uint8_t* dst);
void launch_scatter_bytes(hipStream_t st, const uint8_t* src, const uint32_t* map, size_t rows, uint8_t* dst);

// large G2 linear combinations in two stages (k_msm.hip): per-share affine psi tables + digit codes in HBM
// (tbl: msm_table_bytes, codes: msm_code_bytes), then one 64-step ladder per job.  status: B bytes, jobs with
// status != TC_JOB_OK are skipped (identity out); undecodable operands set TC_JOB_INVALID_ENCODING.
constexpr size_t kMsmMinPoints = 8;  // from here on the Lagrange coefficients come from the one-inversion kernels
// jobs of a share combination that belong to the two-stage path: all of them (null members), or the ones the
// small-index fast path leaves alone -- need: the count k_lagrange made of them (zero: the kernels leave at once)
struct MsmFilter {
  const uint32_t* need = nullptr;
  const uint64_t* idx = nullptr;
  size_t n_per_job = 0, t = 0;
};
size_t msm_table_bytes(size_t n, size_t B);
size_t msm_code_bytes(size_t n, size_t B);
void launch_msm_g2(hipStream_t st, size_t n, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, size_t B,
                   int32_t* tbl, uint8_t* codes, uint8_t* out, uint8_t* status, int nbits = 64, MsmFilter f = MsmFilter());

// the same two stages in G1 (threshold decryption and G1 linear combinations from kMsmMinPoints points on): codes as for G2
// (msm_code_bytes), tables of msm_table_bytes_g1
size_t msm_table_bytes_g1(size_t n, size_t B);
size_t msm_table_jobs_g1(size_t pts_stride, int nbits, size_t B);  // 1 when every job shares ONE point set and the scalars are short
void launch_msm_g1(hipStream_t st, size_t n, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, size_t B, int32_t* tbl,
                   uint8_t* codes, uint8_t* out, uint8_t* status, int nbits = 128);
// the two stages over ragged SEGMENTS of one record array (k_msm.hip k_rec_*, tc_records.h): seg_first / first_chunk are J + 1
// device values each (rec_chunk_ranges), chunks = first_chunk[J]; tbl: rec_table_bytes, codes: rec_code_bytes; `parts` lanes
// (G1) / lane pairs (G2) per segment (rec_parts); status: J bytes as for launch_msm_g2.  launch_rec_gather_keys: keys[r] =
// pks[key_idx[r]], or an undecodable encoding for an index >= K.
size_t rec_table_bytes(bool g2, uint64_t chunks);
size_t rec_code_bytes(uint64_t chunks);
void launch_rec_gather_keys(hipStream_t st, const uint8_t* pks, size_t K, const uint64_t* key_idx, size_t R, uint8_t* keys);
void launch_rec_sum_g2(hipStream_t st, const uint8_t* points, const uint32_t* scalars, const uint64_t* seg_first, const uint64_t* first_chunk, size_t J,
                       uint64_t chunks, size_t parts, int32_t* tbl, uint8_t* codes, uint8_t* out, uint8_t* status, int nbits);
void launch_rec_sum_g1(hipStream_t st, const uint8_t* points, const uint32_t* scalars, const uint64_t* seg_first, const uint64_t* first_chunk, size_t J,
                       uint64_t chunks, size_t parts, int32_t* tbl, uint8_t* codes, uint8_t* out, uint8_t* status, int nbits);
// the PAIRED G1 form (k_rec_*_g1_pair): both sums of every segment, over points_a and over points_b with the same scalars, in one
// stage-T and one stage-L launch; out[2 j] = A_j, out[2 j + 1] = -B_j (J x 2 x 96 bytes); tbl: rec_table_bytes(false, 2 chunks),
// codes: rec_code_bytes(2 chunks); `parts` lanes per SUM; status[j] is set when either half fails
void launch_rec_sum_g1_pair(hipStream_t st, const uint8_t* points_a, const uint8_t* points_b, const uint32_t* scalars, const uint64_t* seg_first,
                            const uint64_t* first_chunk, size_t J, uint64_t chunks, size_t parts, int32_t* tbl, uint8_t* codes, uint8_t* out,
                            uint8_t* status, int nbits);
// random scalars for the batch validation of G1 values: a + b x^2 with a (odd), b from 32-bit draws of ChaCha20(seed, i)
void launch_rlc_scalars_g1(hipStream_t st, const uint8_t* seed32, size_t n, uint8_t* out_fr);

// opt-in operand validation (k_check.hip): valid[i] for point i = (record i / take, sample i % take) of
// records of n_per_job points `stride` bytes apart; launch_invalidate_jobs fails the jobs that own an
// invalid point (status INVALID_ENCODING + identity output, or ok = 0); job j owns record j / group
void launch_subgroup_check_g1(hipStream_t st, const uint8_t* pts, size_t stride, size_t n_per_job, size_t take, size_t n,
                              uint8_t* valid);
void launch_subgroup_check_g2(hipStream_t st, const uint8_t* pts, size_t stride, size_t n_per_job, size_t take, size_t n,
                              uint8_t* valid);
void launch_ok_and_status(hipStream_t st, const uint8_t* status, size_t B, uint8_t* ok);  // ok[j] &= status[j] == OK
void launch_invalidate_jobs(hipStream_t st, const uint8_t* valid, size_t per_job, size_t group, size_t B, uint8_t* status,
                            uint8_t* out, size_t out_bytes, uint8_t* ok);

// ws: the Miller values between the kernels of a check and, for the prepared form, the line buffer of ONE tile of checks
// (k_pairing.hip).  `tile` = checks per pass of the prepared form, sized by the caller from the memory that is free
// (pairing_tile): 61.8 KB of line products per check, 4.05 GB for the full 65 536-check tile.
struct PairingWs {
  int32_t* p;
  size_t tile;
  int form;  // pairing_form's choice for this batch (a PairingForm of k_pairing.hip)
};
int pairing_form(size_t B, const Tuning& tn);          // which kernels run a batch of B checks
bool pairing_form_needs_lines(int form);               // the prepared form: the only one with a line buffer
size_t pairing_tile(size_t B, size_t budget_bytes);    // checks per pass of the prepared form; 0 = the line buffer does not fit
size_t pairing_ws_words(size_t B, size_t tile);
void launch_pairing_check(hipStream_t st, const uint8_t* a, size_t sa, const uint8_t* b, size_t sb, const uint8_t* c,
                          size_t sc, const uint8_t* d, size_t sd, size_t B, uint8_t* ok, PairingWs ws);
// ok[j] = ( prod_{k < n} e(a[j n + k], b[j n + k]) == e(c[j], d[j]) ), or == 1 when c is null: two pairs per lane pair through
// one Miller loop, the values of a job multiplied across lane pairs, ONE final exponentiation per job (k_pairing.hip).
// Strides in bytes per pair, 0 broadcasts one operand.  ws: pairing_product_ws_words(n, B, c != nullptr) words.
size_t pairing_product_ws_words(size_t n, size_t B, bool rhs);
void launch_pairing_product_check(hipStream_t st, const uint8_t* a, size_t sa, const uint8_t* b, size_t sb, size_t n, size_t B, const uint8_t* c,
                                  size_t sc, const uint8_t* d, size_t sd, uint8_t* ok, int32_t* ws);

// fix = false: the hash point WITHOUT its last constant multiplication (tc_gls.h g2_clear_cofactor); the
// caller folds the constant into a scalar (launch_fr_scale_cofactor_fix) or a G1 operand
// (launch_g1_scale_cofactor_fix)
void launch_hash_g2(const Tuning& tn, hipStream_t st, const uint8_t* msgs, const uint64_t* off, size_t B, uint8_t* out, bool fix = true);
void launch_hash_g1_g2(const Tuning& tn, hipStream_t st, const uint8_t* g1, const uint8_t* msgs, const uint64_t* off, size_t B,
                       uint8_t* out, uint8_t* status, bool fix = true);
void launch_fr_scale_cofactor_fix(hipStream_t st, const uint8_t* fr, size_t S, uint8_t* out);
void launch_g1_scale_cofactor_fix(hipStream_t st, const uint8_t* in, size_t stride, size_t n, uint8_t* out);
void launch_xor_with_hash(hipStream_t st, const uint8_t* g1, const uint8_t* data, const uint64_t* off, size_t B,
                          uint8_t* out, uint8_t* status);
void launch_encrypt(hipStream_t st, TableArena ta, const uint8_t* pk, size_t pk_stride, const uint8_t* r, const uint8_t* msgs,
                    const uint64_t* off, size_t B, uint8_t* out_u, uint8_t* out_v, uint8_t* out_w, uint8_t* status);
void launch_commitment_evaluate(hipStream_t st, const uint8_t* commit, size_t t, const uint64_t* idx, size_t M, uint8_t* out,
                                uint8_t* status);
// DKG algebra (k_dkg.hip): the fixed-base window table of the G1 generator is built once per context
size_t fixed_base_table_bytes();
void launch_fixed_base_table(hipStream_t st, int32_t* tbl);
void launch_g1_fixed_base(hipStream_t st, const int32_t* tbl, const uint8_t* fr, size_t M, uint8_t* out, uint8_t* status, int cus);
void launch_bivar_commitment_row(hipStream_t st, const uint8_t* commit, size_t degree, const uint64_t* xs, size_t M, uint8_t* out,
                                 uint8_t* status);
void launch_fr_interpolate(hipStream_t st, size_t n, const uint32_t* xs, const uint32_t* ys, size_t B, uint32_t* out, uint32_t* ws,
                           uint8_t* status);
// DKG verification (k_dkg.hip).  The secret side: coefficients to Montgomery form once (mont: count x 8 words, valid: count
// bytes; the bivariate form expands the (degree+1)(degree+2)/2 coefficients to the full symmetric (degree+1)^2 matrix so
// that every row is contiguous), then one lane per output scalar.
void launch_fr_to_mont(hipStream_t st, const uint8_t* fr, size_t count, uint32_t* mont, uint8_t* valid);
void launch_bivar_to_mont(hipStream_t st, const uint8_t* coeff_fr, size_t degree, uint32_t* mont, uint8_t* valid);
void launch_fr_poly_evaluate(hipStream_t st, const uint32_t* coeff_mont, const uint8_t* coeff_valid, size_t n, const uint8_t* xs_fr, size_t M,
                             size_t B, uint8_t* out_fr, uint8_t* status);
void launch_bivar_poly_row(hipStream_t st, const uint32_t* sq_mont, const uint8_t* sq_valid, size_t degree, const uint64_t* xs, size_t M,
                           uint8_t* out_fr, uint8_t* status);
// the per-job forms of the two G1 Horner kernels: job j's commitment at commits + j * stride (stride 0: one for all) and its
// one abscissa xs[j]; job j's row commitment at rows + j * (degree+1) * 96 and its n abscissae xs[j*n ..], taken by value
void launch_bivar_commitment_row_jobs(hipStream_t st, const uint8_t* commits, size_t stride, size_t degree, const uint64_t* xs, size_t B,
                                      uint8_t* out, uint8_t* status);
void launch_commitment_evaluate_jobs(hipStream_t st, const uint8_t* rows, size_t degree, const uint64_t* xs, size_t n, size_t B, uint8_t* out,
                                     uint8_t* status);
// ok[j] = every one of the per_job points of job j is the same group element in a and b, and all their status bytes are OK
void launch_g1_equal(hipStream_t st, const uint8_t* a, const uint8_t* st_a, const uint8_t* b, const uint8_t* st_b, size_t per_job, size_t B,
                     uint8_t* ok);
// the combined values check: scalars (B x (degree+2) x 8 canonical words; valid: B bytes, 0 = a non-canonical value) from
// tc_dkg.h dkg_rlc_scalar, the points R_j || g1 (B x (degree+2) x 96), and ok[j] = status OK, valid and the sum the identity
void launch_dkg_rlc_scalars(hipStream_t st, const uint8_t* seed32, const uint64_t* xs, const uint8_t* vals_fr, size_t n, size_t degree, size_t B,
                            uint32_t* scalars, uint8_t* valid);
void launch_dkg_rlc_points(hipStream_t st, const uint8_t* rows, size_t degree, const uint8_t* g1_gen, size_t B, uint8_t* out);
void launch_g1_is_identity(hipStream_t st, const uint8_t* pts, const uint8_t* status, const uint8_t* valid, size_t B, uint8_t* ok);
void launch_fill_g1_generator(hipStream_t st, uint8_t* out96, uint8_t* out96_unfix);
// DKG finalisation (k_dkg.hip): out[j] = sum_{k < n, included} pts[k * term_stride + off(j)], off(j) = j * 96 or, column0, the
// position of coefficient (j, 0) of a bivariate commitment; `parts` lanes per output (g1_sum_parts).  mask: n bytes or null;
// member: n x B validity bytes of a membership test or null; term_bad: n zeroed bytes or null, [k] set when an included term k
// is bad.  A failed output is the identity with status INVALID_ENCODING.
size_t g1_sum_parts(size_t B, size_t n, int cus, size_t forced);
void launch_g1_sum(hipStream_t st, bool column0, const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* mask, const uint8_t* member,
                   size_t B, size_t parts, uint8_t* out, uint8_t* status, uint8_t* term_bad);
void launch_fr_sum(hipStream_t st, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* mask, size_t B, uint8_t* out_fr,
                   uint8_t* status);
// out[p] = coefficient 0 of the polynomial through part p's n samples (xs: P x n by value, vals: P x n x 32); status: P bytes
void launch_fr_interpolate_at_zero(hipStream_t st, size_t n, const uint64_t* xs, const uint8_t* vals_fr, const uint8_t* accept, size_t P,
                                   uint8_t* out_fr, uint8_t* status);
void launch_bivar_column0(hipStream_t st, const uint8_t* commits, size_t stride, size_t degree, size_t P, uint8_t* out);
// part_status[p] from the accepted parts' bad points and share statuses (share_st may be null), then identities / zero over
// the outputs (either may be null) when one of them failed
void launch_dkg_generate_verdict(hipStream_t st, const uint8_t* accept, const uint8_t* point_bad, const uint8_t* share_st, size_t P, size_t degree,
                                 uint8_t* part_status, uint8_t* out_commit, uint8_t* out_share);
// DKG resharing (k_dkg.hip): the sums above with one public weight per term.  weights_fr: n x 32 B LE canonical; rec: n x
// wsum_rec_words() words, the weights validated and recoded once per term (launch_wsum_recode) for launch_g1_wsum, which takes
// its lanes per output from g1_wsum_parts.  A non-canonical weight of an included term fails every output.  sel (may be null): n
// term numbers, the sum runs over those terms only (everything else is still addressed by term).
size_t wsum_rec_words();
size_t g1_wsum_parts(size_t B, size_t n, int cus, size_t forced);
void launch_wsum_recode(hipStream_t st, const uint8_t* weights_fr, size_t n, uint32_t* rec);
// slices > 1 (g1_wsum_slices): out = B x slices partial sums, slice-major, with one validity byte each in part_ok -- the caller adds
// them up with launch_g1_sum (term_stride B * 96, n = slices, member = part_ok); slices = 1: out / status are the final ones
size_t g1_wsum_slices(size_t B, size_t n, size_t parts, int cus, size_t forced);
void launch_g1_wsum(hipStream_t st, bool column0, const uint8_t* pts, size_t term_stride, size_t n, const uint32_t* rec, const uint8_t* mask,
                    const uint8_t* member, size_t B, size_t parts, size_t slices, uint8_t* out, uint8_t* status, uint8_t* part_ok,
                    const uint32_t* sel = nullptr);
void launch_fr_wsum(hipStream_t st, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* weights_fr, const uint8_t* mask, size_t B,
                    uint8_t* out_fr, uint8_t* status);
// tc_dkg_reshare_batch.  launch_reshare_check: per part const_st / point_bad / dup (P bytes each) and old_bad (1 byte); member:
// P x (degree+1) verdicts of the first columns' membership test or null, old_member: t_old + 1 or null.  launch_reshare_verdict:
// part_status, then the call's status byte, used (P bytes), the dealers of S (sel_part / sel_idx: t_old + 1 entries) and their
// Lagrange coefficients as weights (P x 32 B, zeroed by the caller); ws: reshare_plan_ws_words(t_old).  launch_reshare_guard:
// identities / zero over the outputs (either may be null) unless the status byte is OK.
void launch_reshare_check(hipStream_t st, const uint8_t* old_commit, const uint8_t* old_member, size_t t_old, const uint64_t* dealer_idx,
                          const uint8_t* commits, size_t stride, size_t degree, const uint8_t* accept, const uint8_t* member, size_t P,
                          uint8_t* const_st, uint8_t* point_bad, uint8_t* dup, uint8_t* old_bad);
size_t reshare_plan_ws_words(size_t t_old);
void launch_reshare_verdict(hipStream_t st, const uint8_t* accept, const uint64_t* dealer_idx, size_t t_old, size_t P, const uint8_t* const_st,
                            const uint8_t* point_bad, const uint8_t* dup, const uint8_t* share_st, const uint8_t* old_bad, uint8_t* part_status,
                            uint8_t* used, uint32_t* sel_part, uint64_t* sel_idx, uint32_t* ws, uint8_t* weights, uint8_t* status);
void launch_reshare_guard(hipStream_t st, const uint8_t* status, size_t degree, uint8_t* out_commit, uint8_t* out_share);

// The robust combiners (k_robust.hip; selection rule in tc_robust.h).  present / bad: jobs x N mask bytes, either may be null.
//   launch_select_shares    idx / slot (jobs x need) = the first `need` eligible slots of every job; enough[j]; the used bytes of a
//                           job that has enough, in row map[j] (null: j) of the caller's B x N array (used may be null)
//   launch_gather_selected  dst (jobs x need x point_bytes) = the selected shares of shares (jobs x N x point_bytes); identities
//                           for a job without enough
//   launch_gather_bytes     dst[r] = src[map[r]]
//   launch_robust_mark      record r = share rec[r] of the caller's arrays with check result ok[r]: the compacted masks
//                           c_present / c_bad (rows bytes each) and the caller's bad[rec[r]] (may be null)
//   launch_robust_finish    status / out / used of the jobs of one pass (job f of the pass = job map[f] of the call, null: f)
//                           from enough, the combine status job_st, the check of the combination ok (null: none) and the
//                           membership bytes of the selected shares (need per job, null: none); verdict[f] (may be null): a
//                           RobustVerdict
void launch_select_shares(hipStream_t st, const uint8_t* present, const uint8_t* bad, size_t N, size_t need, size_t jobs, const uint32_t* map,
                          uint64_t* idx, uint32_t* slot, uint8_t* used, uint8_t* enough);
void launch_gather_selected(hipStream_t st, const uint8_t* shares, size_t N, size_t need, size_t point_bytes, const uint32_t* slot,
                            const uint8_t* enough, size_t jobs, uint8_t* dst);
// the wire forms' replacement of launch_gather_selected (k_mul.hip): shares = jobs x N COMPRESSED encodings (96 / 48 bytes); dst as
// above through the curve-level decode -- no membership test --, ok (jobs x need bytes) = 1 where the record decoded
void launch_decompress_selected(const Tuning& tn, hipStream_t st, bool g2, const uint8_t* shares, size_t N, size_t need, const uint32_t* slot,
                                const uint8_t* enough, size_t jobs, uint8_t* dst, uint8_t* ok);
void launch_gather_bytes(hipStream_t st, const uint8_t* src, const uint32_t* map, size_t rows, uint8_t* dst);
void launch_robust_mark(hipStream_t st, const uint8_t* present, const uint32_t* rec, const uint8_t* ok, size_t rows, uint8_t* c_present,
                        uint8_t* c_bad, uint8_t* bad);
void launch_robust_finish(hipStream_t st, const uint32_t* map, size_t N, size_t need, size_t point_bytes, size_t jobs, const uint8_t* enough,
                          const uint8_t* job_st, const uint8_t* ok, const uint8_t* member, const uint8_t* comb, uint8_t* out, uint8_t* status,
                          uint8_t* used, uint8_t* verdict);

// Blame by bisection (k_blame.hip; rule and bounds in tc_blame.h).
//   launch_blame_seed       seed_out (32 B) = the pass-2 seed of call number `call` under the context's 32-byte key
//   launch_blame_leaves     leaves[i] = [r_(leaf0 + i)] pts[i % period] (period 0: pts[i]; affine encodings, 192 / 96 B) for i < n,
//                           r the 63-bit scalar of launch_rlc_scalars drawn from seed32 at block leaf0 + i; blame_leaf_bytes(g2)
//                           per leaf.  live: n bytes or null; 0 = the identity, and a point that does not decode clears its
//                           byte.  sink: blame_sink_bytes() of scratch.
//   launch_blame_range_sum  out[it] (192 / 96 B affine) = the sum of the leaves [lo[it], hi[it]) of job job[it] (N leaves per
//                           job); `parts` lanes / lane pairs per item (blame_sum_parts)
size_t blame_leaf_bytes(bool g2);
size_t blame_sink_bytes();
void launch_blame_seed(hipStream_t st, const uint8_t* key32, uint64_t call, uint8_t* seed_out);
void launch_blame_leaves(hipStream_t st, TableArena ta, bool g2, const uint8_t* seed32, uint64_t leaf0, const uint8_t* pts, size_t period, uint8_t* live,
                         size_t n, int32_t* leaves, int32_t* sink);
size_t blame_sum_parts(bool g2, size_t n_items, size_t longest, int cus);
void launch_blame_range_sum(hipStream_t st, bool g2, const int32_t* leaves, size_t N, const uint32_t* job, const uint32_t* lo, const uint32_t* hi,
                            size_t n_items, size_t parts, uint8_t* out);

}  // namespace tc
