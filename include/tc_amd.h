/* tc_amd.h -- C ABI of libtc_amd.so: batched BLS12-381 threshold-crypto hot path on MI355X.
 *
 * Drop-in boundary for the data-parallel path of poanetwork/threshold_crypto 0.4.0.  Each
 * entry point is the BATCH form of one reference method (cited below, paths relative to
 * the reference repository); the reference's single-item Rust method maps to a batch of 1.
 * Plain pointers and sizes only; no C++/torch types.  Caller owns every buffer; the library
 * retains no pointer after a call returns (all calls are synchronous unless noted).
 *
 * Encodings (identical to the reference's, so results compare byte-for-byte):
 *   G1 point  : 96 B  uncompressed Zcash form  x || y           (big-endian, flag bits in byte 0)
 *   G2 point  : 192 B uncompressed Zcash form  x.c1||x.c0||y.c1||y.c0
 *               = `into_affine().into_uncompressed()`            (src/lib.rs:89,163,224,238,276)
 *   compressed: 48 B / 96 B = PublicKey::to_bytes / Signature::to_bytes (src/lib.rs:149-153,255-259)
 *   Fr scalar : 32 B little-endian canonical (4 x u64 LE limbs)  (src/serde_impl.rs:296)
 *   share idx : u64, the `T: IntoFr` index of combine_signatures/decrypt (src/into_fr.rs:16-26)
 * Decoding an uncompressed point checks range, flags and the curve equation, and BY DEFAULT every point operand
 * of every entry is also tested for order-r subgroup membership on the device before it is used (what the
 * reference does once per value in from_bytes, src/lib.rs:140-146, 246-252): a job that owns an invalid point
 * fails exactly like one with an undecodable encoding.  The scalar-multiplication and pairing kernels RELY on
 * membership (GLV/GLS ladders through phi = [-x^2] and psi = [x], the psi forms of the share combiner's
 * division, the folded cofactor constant, the 2^-63 bound of the random-linear-combination checks): an on-curve
 * point outside the subgroup would give a result the reference's plain double-and-add does not.  A caller whose
 * operands are KNOWN members -- outputs of this library's own entries, values that entered through
 * tc_g{1,2}_decompress_batch (the reference's checked decode) or were tested with
 * tc_g{1,2}_subgroup_check_batch; typically device-resident data -- opts out with
 * tc_ctx_set_input_checks(ctx, 0) and saves one 64-bit ladder per G2 operand and two per G1 operand.
 *
 * Return value: 0 = TC_OK, < 0 = call-level failure (bad argument / HIP error / no device / host failure);
 * never aborts, never throws across the boundary (every entry is a function-try-block: an exception becomes TC_ERR_HOST).
 * One abort is the ROCm runtime's own -- it kills the process when it cannot allocate a dispatch's private segments -- so a
 * call first compares the free device memory with what its size could ask for (at most ~6.5 GB for a large batch) and
 * returns TC_ERR_HIP instead of launching; TC_PRIVATE_RESERVE=<bytes> in the environment of tc_ctx_create overrides, 0 disables.  Per-job results go to `status[]`
 * (mirrors threshold_crypto::error::Error / FromBytesError, src/error.rs:7-17,37-41) and
 * `ok[]` (the `bool` of the verify methods).
 *
 * I/O residency: by default every data pointer is HOST memory and the call stages through
 * device buffers owned by the context.  After tc_ctx_set_device_io(ctx, 1) every data
 * pointer (inputs, outputs, offsets, status, ok) must be DEVICE memory on the context's GPU,
 * 8-byte aligned, and nothing crosses PCIe.  The kernels read and write them on the CONTEXT's stream and a call returns
 * once they are queued: whatever produced the operands must have finished (or run on the same stream: tc_ctx_set_stream),
 * and results are read after tc_sync or in stream order.  Output buffers should not overlap input buffers: results are written while
 * other jobs' operands are still being read.  The one supported exception is an output that overlaps a POINT operand of the
 * same call job for job (an in-place tc_g{1,2}_mul_batch with S = 1, ok[] over the head of a buffer the call reads): the
 * membership tests of that operand, which otherwise run beside the call's main kernels on the context's second stream, then
 * run in front of them on the main stream.
 *
 * Threading: a context is bound to one GPU and one HIP stream and is thread-compatible (one
 * thread at a time); distinct contexts may be used concurrently (one per GPU, or several on one GPU
 * from several host threads).  Besides its staging buffers a context holds 256 MB of device memory
 * for the per-job ladder tables of the G2 kernels, allocated by the first call that needs them.
 */
#ifndef TC_AMD_H
#define TC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TC_OK 0
#define TC_ERR_INVALID_ARG (-1)
#define TC_ERR_HIP (-2)
#define TC_ERR_NO_DEVICE (-3)
#define TC_ERR_HOST (-4) /* a host-side failure (std::bad_alloc, any C++ exception) stopped at the boundary */

/* per-job status codes */
#define TC_JOB_OK 0
#define TC_JOB_NOT_ENOUGH_SHARES 1 /* Error::NotEnoughShares   src/error.rs:9  */
#define TC_JOB_DUPLICATE_ENTRY 2   /* Error::DuplicateEntry    src/error.rs:12 */
#define TC_JOB_INVALID_ENCODING 3  /* FromBytesError::Invalid  src/error.rs:39 */
#define TC_JOB_SHARE_MISMATCH 4    /* tc_dkg_reshare_batch: a dealer's constant term is not the public key share it holds (no reference error) */

#define TC_G1_BYTES 96
#define TC_G2_BYTES 192
#define TC_G1_COMPRESSED_BYTES 48 /* PK_SIZE  src/lib.rs:71 */
#define TC_G2_COMPRESSED_BYTES 96 /* SIG_SIZE src/lib.rs:75 */
#define TC_FR_BYTES 32

typedef struct tc_ctx tc_ctx;

/* ---- context ---------------------------------------------------------------------------- */
/* Creates a context on HIP device `device`.  Fails with TC_ERR_NO_DEVICE when no gfx950
 * device is visible: there is no CPU fallback. */
int tc_ctx_create(tc_ctx** out, int device);
void tc_ctx_destroy(tc_ctx* ctx);
int tc_ctx_set_device_io(tc_ctx* ctx, int enabled);
int tc_ctx_get_device_io(const tc_ctx* ctx);
/* Use an externally owned HIP stream (hipStream_t passed as void*), e.g. torch's current
 * stream; NULL restores the context's own stream. */
int tc_ctx_set_stream(tc_ctx* ctx, void* hip_stream);
int tc_sync(tc_ctx* ctx);
const char* tc_last_error(const tc_ctx* ctx);
/* Milliseconds spent in the kernels of the most recent call, measured with HIP events on
 * the context's stream (0 if timing is disabled).  tc_ctx_set_timing(ctx, 1) enables it. */
int tc_ctx_set_timing(tc_ctx* ctx, int enabled);
double tc_last_kernel_ms(const tc_ctx* ctx);
/* Checked-input mode (default ON; see "Decoding" above): every uncompressed point operand of every entry is
 * tested for order-r subgroup membership on the device before it is used -- what the reference does once per
 * value in from_bytes (src/lib.rs:140-146, 246-252).  A job that owns an invalid point reports
 * TC_JOB_INVALID_ENCODING / ok = 0, as for an undecodable encoding.  Costs one 64-bit ladder per G2 point
 * (psi(P) = [x]P) and two per G1 point (phi(P) = [-x^2]P).  enabled = 0 is the explicit opt-out for operands the
 * caller knows to be members (this library's own outputs, checked decodes); results on non-members are then
 * unspecified (never memory-unsafe). */
int tc_ctx_set_input_checks(tc_ctx* ctx, int enabled);
int tc_ctx_get_input_checks(const tc_ctx* ctx);
/* A context keeps its staging and table buffers between calls (grow-only; a t = 67 combination of 131 072 jobs holds
 * ~18 GB of per-share tables, sized to a third of the HBM that was free at the call, at most 24 GiB).  tc_ctx_trim
 * waits for the context's stream and gives them back; they are allocated again on demand. */
int tc_ctx_trim(tc_ctx* ctx);
/* Bytes this context's own staging copies have moved over PCIe since it was created (host-I/O mode: every operand up,
 * every result down; device-I/O mode: the 8-byte read-back of off[B] per message-taking call and nothing else). */
int tc_ctx_transfer_bytes(const tc_ctx* ctx, uint64_t* h2d_bytes, uint64_t* d2h_bytes);
/* The form choices this context makes (no counterpart in the reference: a measurement reports which kernels ran).
 * out8[0] / out8[1] = jobs from which a checked G2 decode / a hash takes two jobs per lane pair, out8[2] = the pairing form
 * (0 = by batch size: four lanes per check up to 16 384 checks, the prepared three-kernel form above; 1 quad, 2 lines,
 * 3 pair, 4 fused), out8[3] = bytes the prepared form's line buffer may take (0 = a third of the free HBM), out8[4] = 1 when
 * the membership tests of checked-input mode run on the context's second stream beside the main kernels of a call (default)
 * and 0 when they run before them; out8[5] = bytes the per-share tables of the two-stage kernels may take per call (0 = a third of the
 * free HBM, 1-24 GiB), out8[6] = free device memory a call insists on before its first launch (all ones = by the size of the call,
 * 0 = no check: see "Return value" above); out8[7] = 0 (reserved).  The defaults are the measured choices (csrc/tc_launch.h); the
 * environment variables TC_DUO_MIN, TC_PAIRING_FORM, TC_PAIRING_BUDGET, TC_CHECKS_BESIDE, TC_MSM_BUDGET, TC_PRIVATE_RESERVE (tests,
 * experiments) are read ONCE, by tc_ctx_create -- never on the launch path. */
int tc_ctx_get_tuning(const tc_ctx* ctx, uint64_t* out8);
const char* tc_version(void);

/* ---- hashing onto G2 -------------------------------------------------------------------- */
/* out[j] = hash_g2(msgs[off[j]..off[j+1]])                 pub fn hash_g2, src/lib.rs:691-694 */
int tc_hash_g2_batch(tc_ctx* ctx, const uint8_t* msgs, const uint64_t* off, size_t B, uint8_t* out_g2);
/* out[j] = hash_g1_g2(g1[j], msgs[j])                      fn hash_g1_g2, src/lib.rs:697-707 */
int tc_hash_g1_g2_batch(tc_ctx* ctx, const uint8_t* g1, const uint8_t* msgs, const uint64_t* off, size_t B,
                        uint8_t* out_g2, uint8_t* status);

/* ---- scalar multiplication (share signing / decryption shares) --------------------------- */
/* out[j*S + s] = fr[s] * pts[j]   S signers x B hash points; status[j*S + s].
 * SecretKey::sign_g2 src/lib.rs:372-374, SecretKeyShare::sign_g2 :442-444 */
int tc_g2_mul_batch(tc_ctx* ctx, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, uint8_t* out,
                    uint8_t* status);
/* out[j*n + k] = sk_table[idx[j*n + k]] * hashes[j]: the signature shares of message j by the n signers of its
 * subset, out of a table of N secret key shares (SecretKeyShare::sign_g2 src/lib.rs:442-444 for each selected
 * signer) -- the on-device share generation of the (t, N, batch) workloads, so that nothing larger than the key
 * set crosses PCIe.  An index >= N fails its own output (TC_JOB_INVALID_ENCODING). */
int tc_sign_shares_g2_batch(tc_ctx* ctx, const uint8_t* sk_table, size_t N, const uint64_t* idx, const uint8_t* hashes, size_t n,
                            size_t B, uint8_t* out, uint8_t* status);
/* SecretKeyShare::decrypt_share_no_verify src/lib.rs:460-462, SecretKey::public_key :367-369 */
int tc_g1_mul_batch(tc_ctx* ctx, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, uint8_t* out,
                    uint8_t* status);
/* out[j*n + k] = sk_table[idx[j*n + k]] * u[j]: SecretKeyShare::decrypt_share_no_verify (src/lib.rs:460-462) for
 * the n selected holders of ciphertext j.  status[j*n + k].  u is tested for membership in checked-input mode.
 * The G1 counterpart of tc_sign_shares_g2_batch: an index >= N or a scalar >= r fails its own output
 * (TC_JOB_INVALID_ENCODING, the identity's encoding), an undecodable u the n outputs of its ciphertext.  From enough holders
 * and ciphertexts on (TC_COMB_G1_MIN="<holders>,<batch>" at tc_ctx_create overrides the built-in thresholds) the doublings are
 * done once per ciphertext, on a comb of u (profiles/decrypt_shares_probe.txt). */
int tc_decrypt_shares_g1_batch(tc_ctx* ctx, const uint8_t* sk_table, size_t N, const uint64_t* idx, const uint8_t* u_g1,
                               size_t n, size_t B, uint8_t* out, uint8_t* status);
/* out[j*S + s] = fr[s] * hash_g2(msg[j])   SecretKey::sign :379-381, SecretKeyShare::sign :447-449 */
int tc_sign_batch(tc_ctx* ctx, const uint8_t* fr, const uint8_t* msgs, const uint64_t* off, size_t S, size_t B,
                  uint8_t* out_g2, uint8_t* status);

/* ---- Lagrange combination ------------------------------------------------------------------ */
/* Job j holds n_per_job samples (idx[j*n + k], shares[(j*n + k)*192]) in iteration order (the
 * reference iterates a BTreeMap: ascending index).  As `interpolate` (src/lib.rs:719-767): only
 * the FIRST t+1 samples are used; n_per_job <= t gives status NOT_ENOUGH_SHARES for every job;
 * t == 0 returns the first sample; equal indices are filtered by value from the denominator.
 * PublicKeySet::combine_signatures src/lib.rs:608-615 (t = commit.degree(), :614). */
int tc_combine_g2_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares,
                        size_t B, uint8_t* out, uint8_t* status);
/* Same in G1 (96 B points): the interpolate call of PublicKeySet::decrypt, src/lib.rs:618-625 */
int tc_combine_g1_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares,
                        size_t B, uint8_t* out, uint8_t* status);
/* out[j] = sum_{k < n} scalars[j*n + k] * points[j*n + k]   (scalars 32 B LE, canonical).
 * Commitment::evaluate src/poly.rs:497-508 (= PublicKeySet::public_key_share src/lib.rs:570-573) is
 * this linear combination with scalars (i+1)^k over the commitment coefficients. */
int tc_g1_lincomb_batch(tc_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* points, size_t B, uint8_t* out,
                        uint8_t* status);
int tc_g2_lincomb_batch(tc_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* points, size_t B, uint8_t* out,
                        uint8_t* status);
/* PublicKeySet::decrypt src/lib.rs:618-626: out bytes[off[j]..off[j+1]] = xor_with_hash(combine_g1, v_j) */
int tc_decrypt_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares_g1,
                     const uint8_t* v, const uint64_t* off, size_t B, uint8_t* out, uint8_t* status);
/* `T: IntoFr` beyond u64.  combine_signatures / decrypt are generic over the index type (src/lib.rs:608-622): besides
 * u64 / usize it may be Fr itself or a negative i32 / i64 (src/into_fr.rs:10-14, 28-56: -(|x|) mod r).  idx_fr: B x n_per_job
 * abscissae as 32 B LE canonical Fr values (the IntoFr image; the interpolation point is idx_fr + 1, src/lib.rs:769-773), in
 * the iteration order of the reference's map.  A batch whose first t+1 abscissae per job all fit 64 bits runs the u64
 * kernels (small-index fast path included); otherwise every job takes the general path with coefficients from Fr
 * arithmetic.  A non-canonical abscissa (>= r) fails its job with TC_JOB_INVALID_ENCODING. */
int tc_combine_g2_fr_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint8_t* idx_fr, const uint8_t* shares, size_t B, uint8_t* out,
                           uint8_t* status);
int tc_combine_g1_fr_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint8_t* idx_fr, const uint8_t* shares, size_t B, uint8_t* out,
                           uint8_t* status);
int tc_decrypt_fr_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint8_t* idx_fr, const uint8_t* shares_g1, const uint8_t* v,
                        const uint64_t* off, size_t B, uint8_t* out, uint8_t* status);
/* Wire-level forms of the two combiners.  Shares arrive as they travel -- SignatureShare / Signature::to_bytes, 96 B
 * compressed G2 (src/lib.rs:255-259), DecryptionShare's 48 B compressed G1 (src/serde_impl.rs:174-218) -- and pass through the
 * CHECKED decode of from_bytes (src/lib.rs:140-146, 246-252: flags, range, on the curve, order-r subgroup) on the device:
 * only the first t+1 samples of a job, exactly the ones interpolate() uses; a job that owns an undecodable or non-member
 * share gets TC_JOB_INVALID_ENCODING and the identity.  tc_combine_signatures_wire_batch returns Signature::to_bytes of
 * the combined signature (96 B per job); tc_decrypt_wire_batch the plaintext bytes.  One call = decode + membership +
 * combine + encode on the device; the context's input-check switch does not apply (the decode IS the check). */
int tc_combine_signatures_wire_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares96, size_t B,
                                     uint8_t* out96, uint8_t* status);
int tc_decrypt_wire_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares48, const uint8_t* v,
                          const uint64_t* off, size_t B, uint8_t* out, uint8_t* status);
/* out[j] = data[j] ^ keystream(g1[j])                       fn xor_with_hash, src/lib.rs:710-715 */
int tc_xor_with_hash_batch(tc_ctx* ctx, const uint8_t* g1, const uint8_t* data, const uint64_t* off, size_t B,
                           uint8_t* out, uint8_t* status);

/* ---- pairing checks ------------------------------------------------------------------------ */
/* ok[j] = ( e(a[j], b[j]) == e(c[j], d[j]) ).  A stride of 0 broadcasts one operand to every job;
 * otherwise strides are in bytes (96 / 192 for packed arrays).  An undecodable operand gives 0.
 * PEngine::pairing(..) == PEngine::pairing(..): src/lib.rs:109, :185, :511 */
int tc_pairing_check_batch(tc_ctx* ctx, const uint8_t* a_g1, size_t a_stride, const uint8_t* b_g2, size_t b_stride,
                           const uint8_t* c_g1, size_t c_stride, const uint8_t* d_g2, size_t d_stride, size_t B,
                           uint8_t* ok);
/* ok[j] = ( prod_{k<n} e(a[j*n+k], b[j*n+k]) == 1 ): the product of n >= 1 pairings per job with ONE final exponentiation --
 * the multi-pairing that PEngine::pairing(..) == PEngine::pairing(..) of src/lib.rs:109, :185, :511 is the n = 2 case of (with
 * one G1 operand negated).  a_g1: B x n x 96 B, b_g2: B x n x 192 B, packed.  A pair with an identity operand contributes the
 * factor 1; an undecodable operand gives ok[j] = 0, and so does, in checked-input mode, an operand outside G1 / G2. */
int tc_pairing_product_check_batch(tc_ctx* ctx, const uint8_t* a_g1, const uint8_t* b_g2, size_t n, size_t B, uint8_t* ok);
/* ok[j] = pk.verify_g2(sig[j], hash[j]) = e(pk, hash[j]) == e(g1, sig[j])     src/lib.rs:108-110,170-172 */
int tc_verify_g2_batch(tc_ctx* ctx, const uint8_t* pk_g1, size_t pk_stride, const uint8_t* sig_g2,
                       const uint8_t* hash_g2, size_t B, uint8_t* ok);
/* ok[j] = pk.verify(sig[j], msg[j])                                              src/lib.rs:115-117,177-179 */
int tc_verify_sig_batch(tc_ctx* ctx, const uint8_t* pk_g1, size_t pk_stride, const uint8_t* sig_g2,
                        const uint8_t* msgs, const uint64_t* off, size_t B, uint8_t* ok);
/* OPT-IN fast path for validating the N signature shares of each of B messages against the N public key
 * shares (the loop of examples/threshold_sig.rs:115-131 over PublicKeyShare::verify, src/lib.rs:177-179): per
 * message ONE check  e(sum_i r_i pk_i, H(m)) == e(g1, sum_i r_i sig_i)  with 63-bit r_i (four 16-bit base-|x| digits) drawn from a ChaCha20
 * stream keyed by seed32 (HOST memory in both I/O modes: 32 bytes of fresh secret randomness per call), then
 * per-share checks only for the messages whose combined check failed.  ok[j*N + i] equals
 * PublicKeyShare::verify(pk_i, sig_{j,i}, m_j) except that a message holding an invalid share is accepted as a
 * whole with probability <= 2^-63.  sig_shares: B x N x 192, pk_shares: N x 96; n_fallback (optional, host):
 * number of messages that needed the per-share pass. */
int tc_verify_shares_rlc_batch(tc_ctx* ctx, const uint8_t* pk_shares, size_t N, const uint8_t* sig_shares, const uint8_t* msgs,
                               const uint64_t* off, size_t B, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback);
/* Signature batches under ONE public key by random linear combination (opt-in; BASELINE config 3's shape).  The batch
 * is cut into groups of `group` jobs (0 = 64; at most 1024); a group passes with ONE check
 *     e(pk, sum_j r_j H_j) == e(g1, sum_j r_j sig_j)        instead of `group` checks of src/lib.rs:108-110,
 * r_j = 2^63 secret values from ChaCha20(seed32, j); groups that fail -- or hold an undecodable or non-member operand -- are
 * re-checked job by job, so ok[] equals tc_verify_g2_batch's (pk_stride 0) up to the 2^-63 of a wrongly passing group.
 * *n_fallback (optional) = jobs that went through the per-job checks.  seed32: 32 secret random bytes in HOST memory,
 * drawn after the signatures were received.  tc_verify_sig_rlc_batch hashes the messages on the device first
 * (PublicKey::verify, src/lib.rs:114-117). */
int tc_verify_g2_rlc_batch(tc_ctx* ctx, const uint8_t* pk, const uint8_t* sig, const uint8_t* hash, size_t B, size_t group,
                           const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback);
int tc_verify_sig_rlc_batch(tc_ctx* ctx, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs, const uint64_t* off, size_t B,
                            size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback);
/* Batch verification of RAGGED input (opt-in): M messages, message m owning the records rec_off[m] .. rec_off[m + 1], each
 * record a signature sigs[r] and the index key_idx[r] of its key in a table of K keys -- votes of N validators under their own
 * keys, the shares that have arrived so far, unrelated triples.  ok[r] = pks[key_idx[r]].verify_g2(sigs[r], hashes[m])
 * (PublicKey::verify_g2 / verify, src/lib.rs:108-117; PublicKeyShare::verify, src/lib.rs:177-179; the loop of
 * examples/threshold_sig.rs:115-131 when some shares are missing).  Messages are cut into groups of `group` consecutive
 * messages (0 = 64; at most 1024); a group passes with ONE product check
 *     prod_{m in g} e(P_m, H_m) == e(g1, S_g),   P_m = sum_{r in m} rho_r pks[key_idx[r]],   S_g = sum_{r in g} rho_r sigs[r]
 * rho_r = the 63-bit scalar of ChaCha20(seed32, r): one Miller pair per MESSAGE, one final exponentiation per group and one
 * hash_g2 per message instead of two pairs, one exponentiation and one hash per record.  A group that fails -- or holds an
 * undecodable operand, an index >= K or, in checked-input mode, a non-member -- is re-checked record by record, so ok[] equals
 * tc_verify_g2_batch's (pk_stride 96) on the expanded arrays up to 2^-63 per group; two records whose errors cancel in an
 * unweighted sum are both rejected.  pks: K x 96 B; sigs: R x 192 B, R = rec_off[M] < 2^32; hashes: M x 192 B (msgs / off:
 * one message per m, hashed on the device); rec_off: M + 1 values, 0 first, non-decreasing, in the memory of the other
 * operands; key_idx: R values, or NULL for record r under pks[r] (K >= R); ok: R bytes; seed32: 32 secret random bytes in HOST
 * memory; *n_fallback (optional) = records that went through the per-record checks.  Checked-input mode tests each key TABLE
 * entry, each signature and each hash operand once.  The tables of the two sums take 3 KiB of device memory per record: a
 * call whose tables exceed what tc_g2_lincomb_batch may spend fails with TC_ERR_HIP (split it).  Measured at about 65 536 records
 * against tc_verify_g2_batch on the expanded arrays (profiles/verify_records_probe.txt): 1.17x at 200 keys x 328
 * messages (8x faster than tc_verify_shares_rlc_batch there), SLOWER elsewhere -- 0.82x at 10 keys x 6 553 messages (1.09x behind
 * tc_verify_shares_rlc_batch with hashing on both sides), 0.74x with 30 % of those records missing, 0.90x for 65 536 unrelated
 * triples, 0.53x with a forged record in 1 % of the messages: at this size the launches of the combined form do not fill the GPU. */
int tc_verify_g2_records_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx, const uint8_t* sigs,
                                   const uint64_t* rec_off, const uint8_t* hashes, size_t M, size_t group,
                                   const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback);
int tc_verify_sig_records_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx, const uint8_t* sigs,
                                    const uint64_t* rec_off, const uint8_t* msgs, const uint64_t* off, size_t M, size_t group,
                                    const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback);
/* Decryption-share validation by one random linear combination per ciphertext (opt-in): the loop of
 * examples/threshold_enc.rs over PublicKeyShare::verify_decryption_share (src/lib.rs:182-186) for B ciphertexts x N nodes.
 * pk_shares: N x 96 B (public_key_share(i), the same for every ciphertext); shares: B x N x 96 B; u / v / off / w: the
 * ciphertexts.  ok[j * N + i] = pk_share(i).verify_decryption_share(&shares[j][i], &ct[j]) -- one combined check
 *     e(sum_i r_i share_i, hash_g1_g2(u, v)) == e(sum_i r_i pk_i, w)
 * per ciphertext (r_i: 2^63 secret values from ChaCha20(seed32, .)), share-by-share checks for the ciphertexts whose
 * combined check fails; *n_fallback (optional) = how many did.  seed32: 32 secret random bytes in HOST memory. */
int tc_verify_decryption_shares_rlc_batch(tc_ctx* ctx, const uint8_t* pk_shares, size_t N, const uint8_t* shares, const uint8_t* u,
                                          const uint8_t* v, const uint64_t* off, const uint8_t* w, size_t B, const uint8_t* seed32,
                                          uint8_t* ok, uint64_t* n_fallback);
/* Decryption-share validation of RAGGED input (opt-in; the decryption form of tc_verify_g2_records_rlc_batch): M ciphertexts,
 * ciphertext c owning the records rec_off[c] .. rec_off[c + 1], each record a decryption share shares[r] and the index
 * key_idx[r] of its key in a table of K keys -- the shares a node has received so far for every ciphertext of an epoch, in any
 * number and order.  ok[r] = pks[key_idx[r]].verify_decryption_share(&shares[r], &ct[c]) (PublicKeyShare::verify_decryption_share,
 * src/lib.rs:182-186; the loop of examples/threshold_enc.rs when some shares are missing).  Ciphertexts are cut into groups of
 * `group` consecutive ciphertexts (0 = 64; at most 1024); a group passes with ONE product check
 *     prod_{c in g} e(A_c, H_c) e(-B_c, w_c) == 1,   A_c = sum_{r in c} rho_r shares[r],   B_c = sum_{r in c} rho_r pks[key_idx[r]]
 * H_c = hash_g1_g2(u_c, v_c), rho_r = the 63-bit scalar a + b x^2 of ChaCha20(seed32, r): two Miller pairs per CIPHERTEXT (one
 * lane pair) and one final exponentiation per group instead of two pairs and one exponentiation per record.  A group that
 * fails -- or holds an undecodable operand, an index >= K or, in checked-input mode, a non-member -- is re-checked record by
 * record, so ok[] equals tc_verify_decryption_share_batch's (pk_stride 96) on the expanded arrays up to 2^-63 per group; two
 * records whose errors cancel in an unweighted sum are both rejected.  The result does not depend on Ciphertext::verify (the
 * reference's verify_decryption_share does not call it): an invalid ciphertext makes its honest shares fail.  pks: K x 96 B;
 * shares: R x 96 B, R = rec_off[M] < 2^32; u: M x 96 B, v / off: the M byte strings, w: M x 192 B (the pre-hashed form takes
 * hashes: M x 192 B = hash_g1_g2(u, v), tc_hash_g1_g2_batch, instead of u / v / off); rec_off: M + 1 values, 0 first,
 * non-decreasing, in the memory of the other operands; key_idx: R values, or NULL for record r under pks[r] (K >= R); ok: R
 * bytes; seed32: 32 secret random bytes in HOST memory, drawn after the shares were received; *n_fallback (optional) = records
 * that went through the per-record checks.  Checked-input mode tests each key TABLE entry, each share, each u (each hash in the
 * pre-hashed form) and each w once.  The tables of the two sums take 2 KiB of device memory per record: a call whose tables
 * exceed what tc_g2_lincomb_batch may spend fails with TC_ERR_HIP (split it).  Measured at about 65 536 records against
 * tc_verify_decryption_share_batch on the expanded arrays, hashing on both sides, input checks on / off
 * (profiles/dshare_records_probe.txt): 1.41x / 1.60x at 10 keys x 6 553 ciphertexts, 1.28x / 1.53x with 30 % of
 * those records missing, 1.91x / 2.40x at 200 keys x 328 ciphertexts; SLOWER with a forged record in 1 % of the ciphertexts
 * (0.80x / 0.92x: 48 % of the records go through the second pass at group 64) and level for 65 536 unrelated triples (0.95x /
 * 1.00x).  On DENSE input tc_verify_decryption_shares_rlc_batch stays ahead: the ragged entry runs at 0.79x / 0.95x of it at 10
 * keys, 0.80x / 0.96x at 200 keys, 0.78x / 0.83x with the forged records. */
int tc_verify_decryption_share_records_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx,
                                                 const uint8_t* shares, const uint64_t* rec_off, const uint8_t* u, const uint8_t* v,
                                                 const uint64_t* off, const uint8_t* w, size_t M, size_t group, const uint8_t* seed32,
                                                 uint8_t* ok, uint64_t* n_fallback);
int tc_verify_decryption_share_records_prehashed_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx,
                                                           const uint8_t* shares, const uint64_t* rec_off, const uint8_t* hashes,
                                                           const uint8_t* w, size_t M, size_t group, const uint8_t* seed32, uint8_t* ok,
                                                           uint64_t* n_fallback);
/* ok[j] = Ciphertext(u[j], v[j], w[j]).verify() = e(g1, w) == e(u, hash_g1_g2(u, v))   src/lib.rs:508-512 */
int tc_ciphertext_verify_batch(tc_ctx* ctx, const uint8_t* u_g1, const uint8_t* v, const uint64_t* off,
                               const uint8_t* w_g2, size_t B, uint8_t* ok);
/* Ciphertext::verify (src/lib.rs:508-512) for a batch by random linear combination (opt-in).  The batch is cut into groups of
 * `group` ciphertexts (0 = the default, 64; at most 1024; the last group may be short); a group passes with ONE check
 *     e(g1, sum_j r_j w_j) == prod_j e(r_j u_j, hash_g1_g2(u_j, v_j))
 * -- `group` pairings sharing their Miller-loop squarings two by two and ONE final exponentiation -- instead of `group` checks
 * of two pairings each.  r_j = 2^63 secret values from ChaCha20(seed32, j), pairwise distinct mod r; groups that fail -- or
 * hold an undecodable or, in checked-input mode, non-member operand -- are re-checked ciphertext by ciphertext, so ok[] equals
 * tc_ciphertext_verify_batch's up to the 2^-63 of a wrongly passing group.  The bound assumes u_j in G1 and w_j in G2 (what
 * checked-input mode tests, and what the reference's checked decode guarantees).  *n_fallback (optional, host) = ciphertexts
 * that went through the per-ciphertext checks.  seed32: 32 secret random bytes in HOST memory in both I/O modes, drawn after
 * the ciphertexts were received. */
int tc_ciphertext_verify_rlc_batch(tc_ctx* ctx, const uint8_t* u_g1, const uint8_t* v, const uint64_t* off, const uint8_t* w_g2,
                                   size_t B, size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback);
/* SecretKeyShare::decrypt_share src/lib.rs:452-457 for ONE key share and B ciphertexts: Ciphertext::verify, then [sk] u.
 * ok[j] = 1 and out_g1[j] = the DecryptionShare when ciphertext j is valid; ok[j] = 0 and the identity's encoding when it is
 * not (the reference returns None: an invalid ciphertext never yields a share).  sk_fr: 32 B LE, wiped from the staging
 * buffers after the call.  One call = hash_g1_g2 + pairing check + G1 multiplication, nothing crosses PCIe in between.
 * u and w are tested for membership in G1 / G2 ALWAYS, whatever tc_ctx_set_input_checks says: the pairing check cannot see a
 * small-order component of u, and the secret key must never multiply a point outside the order-r subgroup (the reference's
 * Ciphertext only exists after the checked decode, src/lib.rs:140-146).  A non-canonical sk_fr (>= r) gives ok[j] = 0. */
int tc_decrypt_share_batch(tc_ctx* ctx, const uint8_t* sk_fr, const uint8_t* u_g1, const uint8_t* v, const uint64_t* off,
                           const uint8_t* w_g2, size_t B, uint8_t* out_g1, uint8_t* ok);
/* SecretKeyShare::decrypt_share (src/lib.rs:452-457) for the same holders: Ciphertext::verify ONCE per ciphertext,
 * then the n shares.  ok[j] = 0 -> the n outputs are the identity's encoding.  u and w are tested for membership
 * ALWAYS, as in tc_decrypt_share_batch.  out: B x n x 96 B; status[j*n + k] (may be NULL): a holder's own failure (index >= N,
 * scalar >= r) fails that output only and leaves ok[j] alone. */
int tc_decrypt_shares_batch(tc_ctx* ctx, const uint8_t* sk_table, size_t N, const uint64_t* idx, const uint8_t* u_g1,
                            const uint8_t* v, const uint64_t* off, const uint8_t* w_g2, size_t n, size_t B,
                            uint8_t* out, uint8_t* ok, uint8_t* status);
/* SecretKey::decrypt src/lib.rs:384-391: Ciphertext::verify, g = [sk] u, xor_with_hash(g, v).  out bytes[off[j]..off[j+1]] =
 * the plaintext when ok[j] = 1, zeros when the ciphertext is invalid (None). */
int tc_secret_key_decrypt_batch(tc_ctx* ctx, const uint8_t* sk_fr, const uint8_t* u_g1, const uint8_t* v, const uint64_t* off,
                                const uint8_t* w_g2, size_t B, uint8_t* out, uint8_t* ok);
/* ok[j] = pk_share[j].verify_decryption_share(share[j], ct[j])
 *       = e(share, hash_g1_g2(u, v)) == e(pk_share, w)                                  src/lib.rs:182-186 */
int tc_verify_decryption_share_batch(tc_ctx* ctx, const uint8_t* pk_share_g1, size_t pk_stride,
                                     const uint8_t* share_g1, const uint8_t* u_g1, const uint8_t* v,
                                     const uint64_t* off, const uint8_t* w_g2, size_t B, uint8_t* ok);

/* ---- the steps either side of the path ------------------------------------------------------- */
/* (u[j], v[j], w[j]) = pk.encrypt_with_rng(rng, msg[j]) with the rng's `Fr::random` draw r[j] supplied
 * by the caller (32 B LE): u = r g1, v = msg ^ keystream(r pk), w = r hash_g1_g2(u, v).
 * PublicKey::encrypt_with_rng src/lib.rs:128-137.  v has the layout of msgs (same offsets). */
int tc_encrypt_batch(tc_ctx* ctx, const uint8_t* pk_g1, size_t pk_stride, const uint8_t* r, const uint8_t* msgs,
                     const uint64_t* off, size_t B, uint8_t* out_u, uint8_t* out_v, uint8_t* out_w, uint8_t* status);
/* out[j] = pk_set.public_key_share(idx[j]) = Commitment::evaluate(idx[j] + 1): Horner in G1 over the
 * (t+1) x 96 B commitment.  PublicKeySet::public_key_share src/lib.rs:570-573, src/poly.rs:497-508.
 * With tc_verify_sig_batch (pk_stride = 96) this is the share-validation loop of
 * examples/threshold_sig.rs:115-131 in two launches. */
int tc_public_key_share_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, const uint64_t* idx, size_t M, uint8_t* out,
                              uint8_t* status);

/* ---- robust threshold combination: validate, select and combine in one call ---------------------- */
/* What a node runs per message.  It holds up to N shares, slot i being node i's (abscissa i + 1, public key share
 * Commitment::evaluate(i + 1)); some are absent, some may be forged; it must combine the first t+1 VALID ones and name the
 * peers that sent bad ones.  Common to both entries:
 *   commit    the PublicKeySet's (t+1) x 96 B commitment; commit[0] is the master key.  The N public key shares are computed
 *             on the device once per call.  An undecodable commit -- in checked-input mode also a non-member one -- fails
 *             EVERY job with TC_JOB_INVALID_ENCODING, the identity / zeros, used = bad = 0.
 *   present   B x N bytes, NULL = every share is present.  An absent slot is never used, however malformed its bytes are
 *             (the rule of `mask` in the DKG sums), in checked-input mode too.
 *   used, bad B x N bytes each, optional, zero-initialised by the call.  status: B bytes.
 *   limits    t + 1 <= N and B * N < 2^32; B = 0 is a no-op; a NULL context, or a NULL data pointer with a non-zero size,
 *             answers TC_ERR_INVALID_ARG.  Both entries work in device-I/O mode.
 * The flow is OPTIMISTIC, because a BLS signature (and a combined decryption share) is unique: if ANY t+1 shares combine to
 * something that verifies under the master key, that something is the answer and none of those shares needs a check.
 *  1. A job with fewer than t+1 present slots: TC_JOB_NOT_ENOUGH_SHARES, the identity's encoding, used = bad = 0.
 *  2. Otherwise S0 = the first t+1 present slots in index order.  The job is CLEAN when all S0 shares decode, are group
 *     members (checked-input mode) and their Lagrange combination verifies under commit[0].  Then status OK, out = the
 *     combination, used marks S0, bad = 0.  A clean job makes NO CLAIM ABOUT INDIVIDUAL SHARES: two colluding wrong shares
 *     whose errors cancel in the combination are not reported, and shares past S0 are never examined.
 *  3. A job that is not clean is examined share by share: every present share gets its own check under pk_share(i) (and the
 *     membership test in checked-input mode); bad[j*N + i] = 1 exactly for the present shares that fail it or do not decode.
 *     Fewer than t+1 valid shares: TC_JOB_NOT_ENOUGH_SHARES and the identity (bad is still filled in).  Otherwise used marks
 *     the first t+1 valid shares and out is their combination, which needs no further check.  *n_fallback (optional, host) =
 *     the number of jobs that reached this step.
 * With input checks off the caller vouches that the shares are group members, as for the other combined entries: a pairing
 * cannot see a small-order component (it is killed by the final exponentiation), so a non-member share could pass its
 * check and still spoil the combination. */
/* Signatures: the loop of examples/threshold_sig.rs:115-131 over PublicKeyShare::verify (src/lib.rs:177-179) followed by
 * PublicKeySet::combine_signatures (src/lib.rs:608-615).  sig_shares: B x N x 192.  Exactly one of `hashes` (B x 192 hash
 * points) and `msgs` / `off` (hashed on the device) is given.  out_sig: B x 192.  The combinations of step 2 are verified
 * under the one master key by random linear combination: `group`, `seed32` and the 2^-63 of a wrongly passing group are
 * tc_verify_g2_rlc_batch's (seed32: 32 secret bytes in HOST memory in both I/O modes, wiped from the staging buffers), so
 * the semantics above hold up to that probability. */
int tc_combine_signatures_robust_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present,
                                       const uint8_t* sig_shares, const uint8_t* hashes, const uint8_t* msgs, const uint64_t* off, size_t B,
                                       size_t group, const uint8_t* seed32, uint8_t* out_sig, uint8_t* used, uint8_t* bad, uint8_t* status,
                                       uint64_t* n_fallback);
/* Decryption: the loop of examples/threshold_enc.rs over PublicKeyShare::verify_decryption_share (src/lib.rs:182-186)
 * followed by PublicKeySet::decrypt (src/lib.rs:618-626).  shares_g1: B x N x 96; u / v / off / w: the ciphertexts;
 * out_plain has the layout of v: xor_with_hash(g, v) of a job that ends OK, zeros otherwise.  The check of step 2 is
 * verify_decryption_share of the combination under the master key, e(g, hash_g1_g2(u, v)) == e(commit[0], w), one per job;
 * step 3 the same under pk_share(i).  u and w are tested for membership in checked-input mode, as in
 * tc_verify_decryption_share_batch.  An INVALID CIPHERTEXT (Ciphertext::verify fails, or u / w undecodable or non-member)
 * makes every honest share fail its check: the job ends as TC_JOB_NOT_ENOUGH_SHARES with all present shares marked bad --
 * validate ciphertexts first (tc_ciphertext_verify_batch) when that blame would be acted on. */
int tc_decrypt_robust_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present, const uint8_t* shares_g1,
                            const uint8_t* u_g1, const uint8_t* v, const uint64_t* off, const uint8_t* w_g2, size_t B, uint8_t* out_plain,
                            uint8_t* used, uint8_t* bad, uint8_t* status, uint64_t* n_fallback);
/* The two entries on WIRE BYTES, the form a node receives shares in: sig_shares96 is B x N x 96 (SignatureShare::to_bytes),
 * shares48 is B x N x 48 (compressed G1 decryption shares).  No B x N uncompressed array is made: step 2 decodes only the
 * t+1 shares of S0, straight from the caller's array.  Everything not named below -- commit, hashes, u and w (uncompressed,
 * governed by tc_ctx_set_input_checks), present, used / bad / n_fallback, group / seed32, the limits, B = 0, NULL handling,
 * device-I/O mode, rules 1 and 3, the all-jobs failure on a bad commit, the invalid-ciphertext behaviour -- is as above.
 *   Shares are ALWAYS checked.  They are wire forms: from_bytes semantics (src/lib.rs:246-252, :140-146: on the curve AND in
 *     the order-r subgroup) apply whatever the input-checks setting, as in tc_combine_signatures_wire_batch.
 *   Rule 2, when a job is clean.  Step 2 decodes the S0 shares only as far as the CURVE (flags, range, square root, sign) and
 *     defers membership to the combination C: the job is CLEAN when every share of S0 decodes to a curve point and C decodes
 *     as a curve point, lies in the order-r subgroup and verifies under commit[0] -- one membership ladder per job instead of
 *     t+1.  That acceptance is sound whatever the shares were: the pairing equation under commit[0] has exactly one solution
 *     in G2 (in G1), so a subgroup point that satisfies it IS the master key's signature (IS sk u).  "No claim about
 *     individual shares" now also covers membership: a non-member share inside S0 is reported only if its job reaches step 3,
 *     which happens with overwhelming probability because the cofactor component of a random curve point has large order (its
 *     multiple by a Lagrange coefficient does not vanish, so C is no subgroup point).  The invariant is
 *         status OK  =>  out is the master key's signature / the true plaintext.
 *   Step 3 gives every present share the full checked decode of from_bytes and its own pairing check, so a non-member share
 *     ends as a bad bit there.  A share of S0 that fails even the curve-level decode sends its job to step 3; it is not a job
 *     failure.
 *   Output form.  out_sig96 is B x 96, Signature::to_bytes of the result; a job that does not end OK gets the identity's
 *     compressed encoding (0xC0, then zeros).  out_plain is as above. */
int tc_combine_signatures_robust_wire_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present,
                                            const uint8_t* sig_shares96, const uint8_t* hashes, const uint8_t* msgs, const uint64_t* off, size_t B,
                                            size_t group, const uint8_t* seed32, uint8_t* out_sig96, uint8_t* used, uint8_t* bad, uint8_t* status,
                                            uint64_t* n_fallback);
int tc_decrypt_robust_wire_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present, const uint8_t* shares48,
                                 const uint8_t* u_g1, const uint8_t* v, const uint64_t* off, const uint8_t* w_g2, size_t B, uint8_t* out_plain,
                                 uint8_t* used, uint8_t* bad, uint8_t* status, uint64_t* n_fallback);
/* BLAME BY BISECTION: an opt-in form of step 3 for all four entries, off by default.  Step 3 as written costs a job N pairing
 * checks however few of its shares are bad, so one forged share per message sets the cost of its honest receivers.  With the
 * mode on, every examined share and its public key share are multiplied ONCE by a secret random 63-bit scalar r_i, RANGES of
 * slots are tested with one pairing check each -- e(sum r_i pk_i, H) == e(g1, sum r_i sig_i), for decryption
 * e(sum r_i share_i, H) == e(sum r_i pk_i, w) -- and only the ranges that fail are halved.  A job with k bad shares among N
 * then costs at most min(1 + 2 k d, 2 N - 1) checks in at most 2 d + 1 rounds, d = ceil(log2 N) (17 instead of 200 checks at
 * N = 200, k = 1); the rule is fixed in csrc/tc_blame.h.  The contract:
 *   With the mode on, `out`, `used`, `bad`, `status` and *n_fallback are what the share-by-share step 3 produces, up to
 *     2^-63 per range check (as for the random linear combinations of step 2).  A range that wrongly passes can leave a bad
 *     share unmarked and, because the right half of a failing range whose left half passes is taken to be failing WITHOUT a
 *     check of its own, mark an honest one.
 *   Rules 1 and 2 and the clean-job path are untouched.
 *   Only WHICH pairing checks step 3 runs changes: the checked decode of the wire entries, the per-share membership tests of
 *     checked-input mode, the re-selection and the second combination stay as they are.  A present share that does not decode,
 *     is no group member (where that is tested) or belongs to a job whose own operands are invalid is bad without any check.
 * tc_ctx_set_blame_bisect: key32 == NULL = one pairing check per present share (default); key32 != NULL = blame by bisection.
 * key32: 32 secret random bytes in HOST memory, copied into the context, wiped on destroy / when switched off.  Each robust
 * call derives its own scalars from (key32, a per-context call counter) with ChaCha20 -- never from the caller's seed32, which
 * stays step 2's -- so no scalar is shared between two calls or between the steps: the key must stay secret for the context's
 * lifetime (whoever knows it can forge shares whose errors cancel in a range). */
int tc_ctx_set_blame_bisect(tc_ctx* ctx, const uint8_t* key32);
int tc_ctx_get_blame_bisect(const tc_ctx* ctx); /* 0 / 1; NULL ctx -> 0 */
/* Step 3 of the LAST robust call on this context: pairing checks spent, rounds (host syncs) taken.  Share-by-share mode
 * reports F * N and 1 for F jobs that reached step 3 (0 and 0 when none did).  Either pointer may be NULL. */
int tc_ctx_last_blame_stats(const tc_ctx* ctx, uint64_t* pairing_checks, uint64_t* rounds);

/* ---- DKG algebra (src/poly.rs)----------------------------------------------------------------- */
/* out[i] = coeff_fr[i] * g1: Poly::commitment src/poly.rs:372-377 and BivarPoly::commitment :625-632 (every
 * coefficient times the G1 generator).  Fixed base: a signed 4-bit window table of g1, built once per context
 * and staged in LDS by every workgroup -- 64 mixed additions and no doubling per coefficient. */
int tc_g1_commitment_batch(tc_ctx* ctx, const uint8_t* coeff_fr, size_t M, uint8_t* out, uint8_t* status);
/* BivarCommitment::row src/poly.rs:713-727 for M abscissae: out[m*(degree+1) + i] = sum_j commit[pos(i,j)] * xs[m]^j
 * with commit the (degree+1)(degree+2)/2 coefficients of a symmetric bivariate commitment in coeff_pos order
 * (src/poly.rs:746-750) and xs[m] the u64 `IntoFr` value itself (rows are requested as row(m), m = 0..N).
 * BivarCommitment::evaluate(x, y) :694-710 is row(x) followed by tc_public_key_share_batch-style Horner in y;
 * status[m*(degree+1) + i]. */
int tc_bivar_commitment_row_batch(tc_ctx* ctx, const uint8_t* commit, size_t degree, const uint64_t* xs, size_t M, uint8_t* out,
                                  uint8_t* status);
/* Poly::interpolate src/poly.rs:341-350, 388-417 in Fr: for each of B jobs the n coefficients (low degree first,
 * 32 B LE each; the reference's Poly drops trailing zeros) of the unique polynomial through the n samples
 * (xs[j][k], ys[j][k]) (32 B LE canonical each, abscissae taken as given).  A repeated abscissa -- where the
 * reference panics "sample points must be distinct" -- gives TC_JOB_DUPLICATE_ENTRY and zero coefficients. */
int tc_fr_interpolate_batch(tc_ctx* ctx, size_t n, const uint8_t* xs, const uint8_t* ys, size_t B, uint8_t* out_coeff,
                            uint8_t* status);

/* ---- DKG verification: the secret side and the two checks of `distributed_key_generation` (src/poly.rs:838-878) ----
 * Common to the five entries below.  Abscissae are u64 values taken BY VALUE (the `IntoFr` image of a u64; rows and
 * values are addressed as 1 .. N, 0 and 2^64 - 1 are as good as any).  A non-canonical Fr operand (>= r) fails the
 * outputs that depend on it: TC_JOB_INVALID_ENCODING and a zero output in the two Fr entries, ok = 0 for that value in
 * the check entries (a non-canonical ROW coefficient fails its whole job).  An undecodable point operand fails its whole
 * job, and so does, in checked-input mode (tc_ctx_set_input_checks), a point outside the order-r subgroup.  A size of
 * zero is a no-op (n = 0 in tc_fr_poly_evaluate_batch: the zero polynomial); NULL data pointers with non-zero sizes
 * answer TC_ERR_INVALID_ARG.  The polynomial coefficients, the rows and the values are SECRETS: their staging copies
 * and every temporary derived from them are zeroed before the call returns, and in host-I/O mode so are the staged Fr
 * outputs once they have been copied back.  All five work in device-I/O mode like every other entry. */
/* out[j*M + m] = Poly(coeff[j]).evaluate(xs[m]): Horner in Fr.  src/poly.rs:358-369; SecretKeySet::secret_key_share
 * src/lib.rs:670-673 is evaluate(i + 1).  coeff_fr: B x n x 32 B LE (low degree first), xs_fr: M x 32 B LE shared by
 * every polynomial, out_fr: B x M x 32, status: B x M (optional). */
int tc_fr_poly_evaluate_batch(tc_ctx* ctx, const uint8_t* coeff_fr, size_t n, const uint8_t* xs_fr, size_t M, size_t B,
                              uint8_t* out_fr, uint8_t* status);
/* out[m*(degree+1) + i] = BivarPoly::row(xs[m])[i] = sum_j coeff[pos(i,j)] * xs[m]^j.  src/poly.rs:607-622.
 * coeff_fr: the (degree+1)(degree+2)/2 coefficients in coeff_pos order (src/poly.rs:746-750), 32 B LE each;
 * out_fr: M x (degree+1) x 32; status: M x (degree+1) (optional). */
int tc_bivar_poly_row_batch(tc_ctx* ctx, const uint8_t* coeff_fr, size_t degree, const uint64_t* xs, size_t M, uint8_t* out_fr,
                            uint8_t* status);
/* `row_poly.commitment() == bi_commit.row(m)`, src/poly.rs:841-843, for B parts at once.  Job j: R_j =
 * commit_j.row(xs[j]) (BivarCommitment::row :713-727; written to out_rows, B x (degree+1) x 96, when non-NULL) and
 * ok[j] = 1 iff row_fr[j][i] * g1 == R_j[i] for every i (group elements compare as elements: the identity equals the
 * identity).  commits: job j's (degree+1)(degree+2)/2 x 96 B commitment starts commit_stride BYTES after job j-1's
 * (a multiple of 96, at least the size of one commitment); commit_stride 0 = ONE commitment for every job.
 * row_fr: B x (degree+1) x 32 B LE.  The rows of a failed job with an invalid commitment are the identity's encoding. */
int tc_dkg_verify_rows_batch(tc_ctx* ctx, const uint8_t* commits, size_t commit_stride, size_t degree, const uint64_t* xs,
                             const uint8_t* row_fr, size_t B, uint8_t* out_rows, uint8_t* ok);
/* `bi_commit.evaluate(m, s) == g1 * val`, src/poly.rs:846-848, with evaluate(m, s) = row(m).evaluate(s) (:694-710,
 * :497-508), for B parts of n values each.  Job j holds the row commitment rows[j] ((degree+1) x 96 B, e.g. out_rows
 * above): ok[j*n + k] = 1 iff Commitment(rows[j]).evaluate(xs[j*n + k]) == vals_fr[j*n + k] * g1.
 * xs: B x n, vals_fr: B x n x 32 B LE, ok: B x n. */
int tc_dkg_verify_values_batch(tc_ctx* ctx, const uint8_t* rows, size_t degree, const uint64_t* xs, const uint8_t* vals_fr,
                               size_t n, size_t B, uint8_t* ok);
/* The same ok[] by ONE random linear combination per part (opt-in).  With rho_{j,k} = the first two words of
 * ChaCha20(seed32, block counter j*n + k), low bit set (2^63 equally likely values, pairwise distinct mod r) job j passes
 * -- ok = 1 for all its n values -- when
 *     sum_i (sum_k rho_{j,k} xs_{j,k}^i) * rows[j][i]  -  (sum_k rho_{j,k} vals_{j,k}) * g1  ==  0      (0^0 = 1)
 * which is one G1 linear combination of degree+2 points instead of n Horner chains and n fixed-base multiplications.
 * A job that does not pass -- or holds a non-canonical value or an invalid point -- is re-checked value by value, so its
 * ok[] is tc_dkg_verify_values_batch's; *n_fallback (optional, host) = the number of such jobs.  With rows[j] in G1 a job
 * holding a wrong value passes with probability <= 2^-63; with input checks off the bound assumes members, as for the
 * other combined entries.  seed32: 32 secret random bytes in HOST memory in both I/O modes, drawn after the values were
 * received. */
int tc_dkg_verify_values_rlc_batch(tc_ctx* ctx, const uint8_t* rows, size_t degree, const uint64_t* xs, const uint8_t* vals_fr,
                                   size_t n, size_t B, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback);

/* ---- DKG finalisation: the accepted parts summed into the key set (src/poly.rs:870-876, 895-898) ----
 * Common to the four entries below.  Strides are in BYTES, multiples of the element size (96 / 32) and at least B elements
 * long.  mask / accept: one byte per term / part, in the same memory as the other data pointers; NULL = all.  A term whose
 * byte is 0 is EXCLUDED: it is not decoded and touches neither output nor status, however malformed its bytes are -- a
 * rejected dealer's commitment may be garbage -- also in checked-input mode.  An included point that does not decode, or, in
 * checked-input mode, lies outside the order-r subgroup, fails its output: the identity's encoding and
 * TC_JOB_INVALID_ENCODING; an included non-canonical Fr value: zero and TC_JOB_INVALID_ENCODING.  n = 0, or every term
 * excluded: the identity / zero with status OK.  B = 0 or P = 0 is a no-op; NULL data pointers with non-zero sizes answer
 * TC_ERR_INVALID_ARG; status is optional.  Fr operands are SECRETS: staging copies, temporaries derived from them and, in
 * host-I/O mode, the staged Fr outputs are zeroed.  All four work in device-I/O mode.  A G1 output is split over the lanes
 * of a wave when the batch alone would leave the GPU empty; the bytes do not depend on the split (TC_SUM_PARTS forces it). */
/* out[j] = sum_{k<n, included} pts[k*term_stride + j*96]: Commitment::add_assign (src/poly.rs:462-471) folded over n
 * commitments of B coefficients each (the caller pads a shorter one with the identity). */
int tc_g1_sum_batch(tc_ctx* ctx, const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* mask, size_t B, uint8_t* out,
                    uint8_t* status);
/* out[i] = sum_{p<P, included} commits[p][coeff_pos(i,0)], i <= degree: `sum_commit += bi_commit.row(0)` (src/poly.rs:895-898;
 * row(0)[i] is coefficient (i,0): no multiplication).  commit_stride as in tc_dkg_verify_rows_batch (never 0 here).
 * out: (degree+1) x 96, status: degree+1. */
int tc_bivar_commitment_row0_sum_batch(tc_ctx* ctx, const uint8_t* commits, size_t commit_stride, size_t degree, size_t P,
                                       const uint8_t* mask, uint8_t* out, uint8_t* status);
/* out[j] = sum_{k<n, included} vals[k*term_stride + j*32] mod r: Poly::add_assign (src/poly.rs:68-80) per coefficient, and
 * `sec_keys[m - 1].add_assign(..)` :876.  SECRET operands and outputs. */
int tc_fr_sum_batch(tc_ctx* ctx, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* mask, size_t B,
                    uint8_t* out_fr, uint8_t* status);
/* The finalisation in one call (src/poly.rs:870-876 and :895-898 over the accepted parts).  out_commit ((degree+1) x 96, may
 * be NULL) = the row-0 sum of the accepted parts' commitments: the PublicKeySet's commitment.  out_share_fr (32 B, may be
 * NULL: an observer without a secret; xs and vals_fr are then ignored) = sum over the accepted parts of
 * `my_row.evaluate(0)`, my_row the polynomial through part p's n_v samples (xs[p*n_v + k] by value, vals_fr[(p*n_v + k)*32]):
 * the node's SecretKeyShare.  part_status[p] (optional) of an accepted part: OK, TC_JOB_INVALID_ENCODING for a bad or
 * non-member first-column point or a non-canonical value, TC_JOB_DUPLICATE_ENTRY for a repeated abscissa; a rejected part is
 * OK and is never used.  If any accepted part fails, out_commit is degree+1 identity encodings and out_share_fr is zero --
 * never a partial key -- and the call still returns TC_OK. */
int tc_dkg_generate_batch(tc_ctx* ctx, const uint8_t* commits, size_t commit_stride, size_t degree, size_t P,
                          const uint8_t* accept, const uint64_t* xs, const uint8_t* vals_fr, size_t n_v, uint8_t* out_commit,
                          uint8_t* out_share_fr, uint8_t* part_status);

/* ---- DKG resharing: a new validator set, the SAME master key ----
 * The old holders of shares deal; the messages are the DKG's and are checked by tc_dkg_verify_rows_batch /
 * tc_dkg_verify_values_batch as they are.  The finalisation weights dealer p by the Lagrange coefficient at zero of its
 * abscissa (the coefficients of src/lib.rs:719-767) instead of 1, so `Poly * Fr` (src/poly.rs:210-254) and
 * Commitment::add_assign (src/poly.rs:462-471) take the places of the plain sums of src/poly.rs:870-876 and :895-898.
 * The rules of the finalisation entries above (strides, mask, checked-input mode on INCLUDED terms only, identity and empty
 * cases, secrets, device-I/O) carry over.  weights_fr: n x 32 B little-endian canonical, PUBLIC, shared by all outputs; an
 * included term whose weight is not canonical (>= r) fails EVERY output; the weight of an excluded term is not looked at. */
/* out[j] = sum_{k<n, included} weights[k] * pts[k*term_stride + j*96].  Each product is tc_g1_mul_batch's ladder; the products
 * are added with the complete formulas, so weights[a]*pts[a] == +-weights[b]*pts[b] is an ordinary input. */
int tc_g1_weighted_sum_batch(tc_ctx* ctx, const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* weights_fr,
                             const uint8_t* mask, size_t B, uint8_t* out, uint8_t* status);
/* out[j] = sum_{k<n, included} weights[k] * vals[k*term_stride + j*32] mod r.  vals and out are SECRETS, as in tc_fr_sum_batch. */
int tc_fr_weighted_sum_batch(tc_ctx* ctx, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* weights_fr,
                             const uint8_t* mask, size_t B, uint8_t* out_fr, uint8_t* status);
/* The finalisation of a resharing in one call.  old_commit ((t_old+1) x 96): the commitment of the key set being handed over;
 * old node i holds f(i+1) and its public key share is old_commit.evaluate(i+1) (src/poly.rs:497-508).  Part p is dealt by old
 * node dealer_idx[p] (P x u64): a symmetric bivariate polynomial of the NEW degree whose constant term is that node's share.
 * commits, commit_stride, accept, xs, vals_fr, n_v, out_commit, out_share_fr (NULL: an observer) and part_status are
 * tc_dkg_generate_batch's.  S = the first t_old+1 accepted parts in part order (the `take(t + 1)` of src/lib.rs:719-767),
 * lambda_p = the Lagrange coefficient at zero of abscissa dealer_idx[p]+1 within S:
 *     out_commit[i] = sum_{p in S} lambda_p * commits[p][coeff_pos(i,0)]     out_share = sum_{p in S} lambda_p * F_p(m, 0)
 * so out_commit[0] == old_commit[0].  used (P bytes, optional) marks S; status: ONE byte (optional).  In this order:
 *  1. old_commit does not decode (checked-input mode: or holds a non-member): status = TC_JOB_INVALID_ENCODING, every
 *     part_status OK, used = 0, the outputs guarded.
 *  2. A rejected part is never read and stays OK.
 *  3. EVERY accepted part is examined, not only S -- the blame is complete and equal at all nodes.  First match:
 *     TC_JOB_INVALID_ENCODING  a first-column point that does not decode (checked mode: or is no member), a non-canonical value
 *     TC_JOB_DUPLICATE_ENTRY   dealer_idx[p] repeats that of an earlier accepted part; an abscissa repeats in its samples
 *     TC_JOB_SHARE_MISMATCH    commits[p][coeff_pos(0,0)] != old_commit.evaluate(dealer_idx[p]+1), as group elements
 *  4. Any accepted part not OK: status = the code of the first such part, used = 0, the outputs guarded.
 *  5. Otherwise fewer than t_old+1 accepted parts: status = TC_JOB_NOT_ENOUGH_SHARES, the outputs guarded.
 *  6. Otherwise used marks S, the outputs are as above, status = TC_JOB_OK.
 * Guarded: degree+1 identity encodings and a zero share, never a partial key.  The call returns TC_OK in all these cases.
 * Only the first columns are read.  P = 0 is a no-op; t_old, degree < 4096, P < 65536. */
int tc_dkg_reshare_batch(tc_ctx* ctx, const uint8_t* old_commit, size_t t_old, const uint64_t* dealer_idx, const uint8_t* commits,
                         size_t commit_stride, size_t degree, size_t P, const uint8_t* accept, const uint64_t* xs,
                         const uint8_t* vals_fr, size_t n_v, uint8_t* out_commit, uint8_t* out_share_fr, uint8_t* used,
                         uint8_t* part_status, uint8_t* status);

/* ---- membership tests ------------------------------------------------------------------------ */
/* ok[j] = 1 iff pts[j] decodes (range, flags, curve equation) and lies in the order-r subgroup: the
 * CHECKED half of `into_affine` (from_bytes, src/lib.rs:140-146, 246-252) for values that arrive
 * uncompressed.  The identity is a member. */
int tc_g1_subgroup_check_batch(tc_ctx* ctx, const uint8_t* pts96, size_t B, uint8_t* ok);
int tc_g2_subgroup_check_batch(tc_ctx* ctx, const uint8_t* pts192, size_t B, uint8_t* ok);

/* ---- wire formats --------------------------------------------------------------------------- */
/* uncompressed -> compressed: PublicKey::to_bytes src/lib.rs:149-153, Signature::to_bytes :255-259 */
int tc_g1_compress_batch(tc_ctx* ctx, const uint8_t* in96, size_t B, uint8_t* out48, uint8_t* status);
int tc_g2_compress_batch(tc_ctx* ctx, const uint8_t* in192, size_t B, uint8_t* out96, uint8_t* status);

/* compressed -> uncompressed with the CHECKED decode of PublicKey::from_bytes src/lib.rs:140-146 and
 * Signature::from_bytes :246-252 (serde: src/serde_impl.rs:187-218): flags, range, on-curve and
 * order-r subgroup membership; status = TC_JOB_INVALID_ENCODING (FromBytesError::Invalid) otherwise. */
int tc_g1_decompress_batch(tc_ctx* ctx, const uint8_t* in48, size_t B, uint8_t* out96, uint8_t* status);
int tc_g2_decompress_batch(tc_ctx* ctx, const uint8_t* in96, size_t B, uint8_t* out192, uint8_t* status);

/* ---- several GPUs of one node from ONE host process ------------------------------ */
/* A group owns one tc_ctx and one worker thread per GPU.  Jobs are independent, so a batch in host memory is
 * split into contiguous ranges, one per GPU, and there is no data-path collective; the two exchange steps of the
 * path run on RCCL (bound with dlopen at tc_group_create): the BROADCAST of the key-set parameters from rank 0 to
 * every GPU's HBM over xGMI (tc_group_set_keyset) and the ALL-REDUCE of the per-GPU valid counts
 * (tc_group_verify_g2).  Processes that prefer one process per GPU use a plain tc_ctx each and do the broadcast
 * themselves (torch.distributed / RCCL: threshold_crypto_amd/parallel.py, bench.py --gpus N).
 * devices: ndev HIP device ids; duplicate ids put several ranks on one GPU (no RCCL then: a test configuration). */
typedef struct tc_group tc_group;
int tc_group_create(tc_group** out, const int* devices, int ndev);
void tc_group_destroy(tc_group* g);
int tc_group_size(const tc_group* g);
int tc_group_uses_rccl(const tc_group* g);
tc_ctx* tc_group_ctx(tc_group* g, int rank);             /* the rank's context, for direct tc_*_batch calls */
const char* tc_group_last_error(const tc_group* g);
/* contiguous range [start, start + count) of a B-job batch that rank `rank` works on */
int tc_group_shard(const tc_group* g, size_t B, int rank, size_t* start, size_t* count);
/* bytes that crossed PCIe since the group was created: the group's own copies plus its contexts' staging copies */
int tc_group_transfer_bytes(const tc_group* g, uint64_t* h2d_bytes, uint64_t* d2h_bytes);
/* PublicKeySet { commit } src/lib.rs:539-543: (t+1) x 96 B from host memory to rank 0, then RCCL broadcast */
int tc_group_set_keyset(tc_group* g, size_t t, const uint8_t* commit);
int tc_group_get_keyset(tc_group* g, int rank, uint8_t* out_commit);
/* PublicKeySet::combine_signatures src/lib.rs:608-615 for B jobs (host buffers), threshold = the key set's */
int tc_group_combine_signatures(tc_group* g, size_t n_per_job, const uint64_t* idx, const uint8_t* shares, size_t B, uint8_t* out,
                                uint8_t* status);
/* PublicKeySet::public_key().verify_g2 src/lib.rs:565-567, 108-110 for B jobs; n_valid (optional): all-reduced count */
int tc_group_verify_g2(tc_group* g, const uint8_t* sig, const uint8_t* hash, size_t B, uint8_t* ok, uint64_t* n_valid);
/* BASELINE config 5 in one call: hash each message, sign the n shares of its signer subset ON the device from the
 * N x 32 B table of secret key shares, combine, verify under the master key.  idx: B x n ascending signer indices.
 * Per rank only its slice of msgs / off / idx and the share table go up and its slice of sig / ok comes back; the hash
 * points and the B x n x 192 B of share signatures are made and consumed in the rank's HBM (persistent per-rank device
 * buffers, one persistent worker thread per GPU).  off must start at 0 and be non-decreasing (checked before sharding). */
int tc_group_sign_combine_verify(tc_group* g, const uint8_t* sk_table, size_t N, const uint64_t* idx, size_t n, const uint8_t* msgs,
                                 const uint64_t* off, size_t B, uint8_t* sig, uint8_t* ok, uint64_t* n_valid);

#ifdef __cplusplus
}
#endif
#endif /* TC_AMD_H */
