// gfx950 kernels: DKG algebra (tc_dkg.h) -- fixed-base commitments from an LDS-resident window table of the
// G1 generator, rows of bivariate commitments, Fr interpolation, and the DKG verification kernels: Fr rows and values, the
// per-job forms of the two G1 Horner kernels, the comparisons and the scalars of the combined values check, and the DKG
// finalisation: sums of G1 points split over the lanes of a wave, sums of Fr values, interpolation at zero; and the resharing:
// the same sums with one public weight per term, the dealers' constant check, the selection and the verdict.
#include "tc_dkg.h"
#include "tc_launch.h"

namespace tc {

constexpr int kFbBlock = 256;  // four waves share one LDS copy of the table; two such workgroups per CU

__global__ void k_fixed_base_table(int32_t* __restrict__ tbl) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e < kFbWindows * kFbEntries) fixed_base_table_entry(e, tbl + (size_t)e * kFbPointWords);
}

// out[j] = fr[j] * g1.  Persistent workgroups: each stages the 56 KB table in LDS once (coalesced 16-byte
// loads) and then walks the batch with a grid stride; every addition reads its table entry with ds_read.
__global__ __launch_bounds__(kFbBlock, 2) void k_g1_fixed_base(const int32_t* __restrict__ tbl_g, const uint8_t* __restrict__ fr,
                                                              size_t M, uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  __shared__ int32_t tbl[kFbTableWords];
  {
    const int4* src = reinterpret_cast<const int4*>(tbl_g);
    int4* dst = reinterpret_cast<int4*>(tbl);
    for (int i = threadIdx.x; i < kFbTableWords / 4; i += kFbBlock) dst[i] = src[i];
  }
  __syncthreads();
  for (size_t base = (size_t)blockIdx.x * kFbBlock; base < M; base += (size_t)gridDim.x * kFbBlock) {
    const size_t j = base + threadIdx.x;
    if (j < M) {
      const uint8_t st = job_g1_fixed_base_mul((const int32_t*)tbl, fr + j * 32, out + j * 96);
      if (status) status[j] = st;
    }
  }
}

// out[(m * (degree + 1) + i)] = BivarCommitment::row(xs[m])[i]
__global__ __launch_bounds__(kBlock, TC_WAVES_G1_AUX) void k_bivar_commitment_row(const uint8_t* __restrict__ commit, size_t degree,
                                                                            const uint64_t* __restrict__ xs, size_t M,
                                                                            uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t n = degree + 1;
  if (tid >= M * n) return;
  const size_t m = tid / n, i = tid % n;
  const uint8_t st = job_bivar_commitment_row(commit, degree, i, xs[m], out + tid * 96);
  if (status) status[tid] = st;
}

__global__ __launch_bounds__(kBlock, TC_WAVES_G1) void k_fr_interpolate(size_t n, const uint32_t* __restrict__ xs, const uint32_t* __restrict__ ys,
                                                                      size_t B, uint32_t* __restrict__ out, uint32_t* __restrict__ ws,
                                                                      uint8_t* __restrict__ status) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= B) return;
  const uint8_t st = job_fr_interpolate(n, xs + j * n * 8, ys + j * n * 8, out + j * n * 8, ws + j * 2 * (n + 1) * 8);
  if (status) status[j] = st;
}

size_t fixed_base_table_bytes() { return (size_t)kFbTableWords * sizeof(int32_t); }
void launch_fixed_base_table(hipStream_t st, int32_t* tbl) {
  hipLaunchKernelGGL(k_fixed_base_table, dim3(grid_for(kFbWindows * kFbEntries)), dim3(kBlock), 0, st, tbl);
}
void launch_g1_fixed_base(hipStream_t st, const int32_t* tbl, const uint8_t* fr, size_t M, uint8_t* out, uint8_t* status, int cus) {
  if (!M) return;
  size_t blocks = (M + kFbBlock - 1) / kFbBlock;
  const size_t resident = (size_t)(cus > 0 ? cus : 256) * 2;  // two workgroups per CU hold their LDS tables at once
  if (blocks > resident) blocks = resident;
  hipLaunchKernelGGL(k_g1_fixed_base, dim3((unsigned)blocks), dim3(kFbBlock), 0, st, tbl, fr, M, out, status);
}
void launch_bivar_commitment_row(hipStream_t st, const uint8_t* commit, size_t degree, const uint64_t* xs, size_t M, uint8_t* out,
                                 uint8_t* status) {
  const size_t n = M * (degree + 1);
  if (n) hipLaunchKernelGGL(k_bivar_commitment_row, dim3(grid_for(n)), dim3(kBlock), 0, st, commit, degree, xs, M, out, status);
}
void launch_fr_interpolate(hipStream_t st, size_t n, const uint32_t* xs, const uint32_t* ys, size_t B, uint32_t* out, uint32_t* ws,
                           uint8_t* status) {
  if (B) hipLaunchKernelGGL(k_fr_interpolate, dim3(grid_for(B)), dim3(kBlock), 0, st, n, xs, ys, B, out, ws, status);
}

// ---- DKG verification (tc_dkg.h) ------------------------------------------------------------------------------
// the secret side: every coefficient to Montgomery form ONCE, then one lane per output scalar
__global__ __launch_bounds__(kBlock) void k_fr_to_mont(const uint8_t* __restrict__ fr, size_t count, uint32_t* __restrict__ mont,
                                                       uint8_t* __restrict__ valid) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  valid[t] = fr_mont_from_le32(fr + t * 32, mont + t * 8) ? 1 : 0;
}
// sq[i][j] = coeff[pos(i, j)]: the symmetric matrix in full, so that row i is a contiguous polynomial
__global__ __launch_bounds__(kBlock) void k_bivar_to_mont(const uint8_t* __restrict__ coeff, size_t degree, uint32_t* __restrict__ mont,
                                                          uint8_t* __restrict__ valid) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t n = degree + 1;
  if (t >= n * n) return;
  valid[t] = fr_mont_from_le32(coeff + bivar_coeff_pos(t / n, t % n) * 32, mont + t * 8) ? 1 : 0;
}
// out[j * M + m] = Poly(coeff[j]).evaluate(xs[m])
__global__ __launch_bounds__(kBlock) void k_fr_poly_evaluate(const uint32_t* __restrict__ coeff_mont, const uint8_t* __restrict__ coeff_valid,
                                                             size_t n, const uint8_t* __restrict__ xs, size_t M, size_t B,
                                                             uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= B * M) return;
  const size_t j = t / M, m = t % M;
  const uint8_t st = job_fr_poly_evaluate(coeff_mont + j * n * 8, coeff_valid + j * n, n, xs + m * 32, out + t * 32);
  if (status) status[t] = st;
}
// out[m * (degree + 1) + i] = BivarPoly::row(xs[m])[i]
__global__ __launch_bounds__(kBlock) void k_bivar_poly_row(const uint32_t* __restrict__ sq_mont, const uint8_t* __restrict__ sq_valid, size_t degree,
                                                           const uint64_t* __restrict__ xs, size_t M, uint8_t* __restrict__ out,
                                                           uint8_t* __restrict__ status) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t n = degree + 1;
  if (t >= M * n) return;
  const uint8_t st = job_bivar_poly_row(sq_mont, sq_valid, degree, t % n, xs[t / n], out + t * 32);
  if (status) status[t] = st;
}

// k_bivar_commitment_row with one commitment and one abscissa PER JOB: out[j * (degree + 1) + i] = commit_j.row(xs[j])[i]
__global__ __launch_bounds__(kBlock, TC_WAVES_G1_AUX) void k_bivar_commitment_row_jobs(const uint8_t* __restrict__ commits, size_t stride,
                                                                                      size_t degree, const uint64_t* __restrict__ xs, size_t B,
                                                                                      uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t n = degree + 1;
  if (tid >= B * n) return;
  const size_t j = tid / n, i = tid % n;
  status[tid] = job_bivar_commitment_row(commits + j * stride, degree, i, xs[j], out + tid * 96);
}
// k_commitment_evaluate (k_hash.hip) with one commitment per job and the abscissa by value:
// out[j * n + k] = Commitment(rows[j]).evaluate(xs[j * n + k])
__global__ __launch_bounds__(kBlock, TC_WAVES_G1_AUX) void k_commitment_evaluate_jobs(const uint8_t* __restrict__ rows, size_t degree,
                                                                                     const uint64_t* __restrict__ xs, size_t n, size_t B,
                                                                                     uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (tid >= B * n) return;
  status[tid] = job_commitment_evaluate_at(rows + (tid / n) * (degree + 1) * 96, degree, xs[tid], out + tid * 96);
}
// ok[j] = the per_job points of job j are the same group elements in a and b.  Both sides are this library's own canonical
// encodings (the identity: 0x40 and zeros), so equal elements are equal bytes; a failed status on either side is "not equal".
__global__ __launch_bounds__(kBlock) void k_g1_equal(const uint8_t* __restrict__ a, const uint8_t* __restrict__ st_a, const uint8_t* __restrict__ b,
                                                     const uint8_t* __restrict__ st_b, size_t per_job, size_t B, uint8_t* __restrict__ ok) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= B) return;
  bool good = true;
  for (size_t i = j * per_job; i < (j + 1) * per_job; i++) {
    good = good && st_a[i] == TC_JOB_OK && st_b[i] == TC_JOB_OK;
    const uint64_t* pa = reinterpret_cast<const uint64_t*>(a + i * 96);
    const uint64_t* pb = reinterpret_cast<const uint64_t*>(b + i * 96);
    for (int w = 0; w < 12; w++) good = good && pa[w] == pb[w];
  }
  ok[j] = good ? 1 : 0;
}

// the combined values check: one lane per scalar (job j, i = 0 .. degree + 1); the lane of c_g sees the values and owns valid[j]
__global__ __launch_bounds__(kBlock) void k_dkg_rlc_scalars(const uint8_t* __restrict__ seed32, const uint64_t* __restrict__ xs,
                                                            const uint8_t* __restrict__ vals, size_t n, size_t degree, size_t B,
                                                            uint32_t* __restrict__ scalars, uint8_t* __restrict__ valid) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t per = degree + 2;
  if (t >= B * per) return;
  const size_t j = t / per, i = t % per;
  uint32_t key[8];
  for (int w = 0; w < 8; w++)
    key[w] = (uint32_t)seed32[4 * w] | ((uint32_t)seed32[4 * w + 1] << 8) | ((uint32_t)seed32[4 * w + 2] << 16) | ((uint32_t)seed32[4 * w + 3] << 24);
  const bool good = dkg_rlc_scalar(key, j, n, degree, xs + j * n, vals + j * n * 32, i, scalars + t * 8);
  if (i == degree + 1) valid[j] = good ? 1 : 0;
}
// out[j] = rows[j] || g1, one 8-byte word per lane
__global__ __launch_bounds__(kBlock) void k_dkg_rlc_points(const uint8_t* __restrict__ rows, size_t degree, const uint8_t* __restrict__ g1_gen, size_t B,
                                                           uint8_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t row_words = (degree + 1) * 12, per = row_words + 12;
  if (t >= B * per) return;
  const size_t j = t / per, w = t % per;
  reinterpret_cast<uint64_t*>(out)[t] = w < row_words ? reinterpret_cast<const uint64_t*>(rows)[j * row_words + w]
                                                      : reinterpret_cast<const uint64_t*>(g1_gen)[w - row_words];
}
__global__ __launch_bounds__(kBlock) void k_g1_is_identity(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ status,
                                                           const uint8_t* __restrict__ valid, size_t B, uint8_t* __restrict__ ok) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= B) return;
  ok[j] = (status[j] == TC_JOB_OK && valid[j] != 0 && (pts[j * 96] & 0x40) != 0) ? 1 : 0;
}

void launch_fr_to_mont(hipStream_t st, const uint8_t* fr, size_t count, uint32_t* mont, uint8_t* valid) {
  if (count) hipLaunchKernelGGL(k_fr_to_mont, dim3(grid_for(count)), dim3(kBlock), 0, st, fr, count, mont, valid);
}
void launch_bivar_to_mont(hipStream_t st, const uint8_t* coeff_fr, size_t degree, uint32_t* mont, uint8_t* valid) {
  const size_t n = (degree + 1) * (degree + 1);
  hipLaunchKernelGGL(k_bivar_to_mont, dim3(grid_for(n)), dim3(kBlock), 0, st, coeff_fr, degree, mont, valid);
}
void launch_fr_poly_evaluate(hipStream_t st, const uint32_t* coeff_mont, const uint8_t* coeff_valid, size_t n, const uint8_t* xs_fr, size_t M,
                             size_t B, uint8_t* out_fr, uint8_t* status) {
  if (B * M) hipLaunchKernelGGL(k_fr_poly_evaluate, dim3(grid_for(B * M)), dim3(kBlock), 0, st, coeff_mont, coeff_valid, n, xs_fr, M, B, out_fr, status);
}
void launch_bivar_poly_row(hipStream_t st, const uint32_t* sq_mont, const uint8_t* sq_valid, size_t degree, const uint64_t* xs, size_t M,
                           uint8_t* out_fr, uint8_t* status) {
  const size_t n = M * (degree + 1);
  if (n) hipLaunchKernelGGL(k_bivar_poly_row, dim3(grid_for(n)), dim3(kBlock), 0, st, sq_mont, sq_valid, degree, xs, M, out_fr, status);
}
void launch_bivar_commitment_row_jobs(hipStream_t st, const uint8_t* commits, size_t stride, size_t degree, const uint64_t* xs, size_t B,
                                      uint8_t* out, uint8_t* status) {
  const size_t n = B * (degree + 1);
  if (n) hipLaunchKernelGGL(k_bivar_commitment_row_jobs, dim3(grid_for(n)), dim3(kBlock), 0, st, commits, stride, degree, xs, B, out, status);
}
void launch_commitment_evaluate_jobs(hipStream_t st, const uint8_t* rows, size_t degree, const uint64_t* xs, size_t n, size_t B, uint8_t* out,
                                     uint8_t* status) {
  if (B * n) hipLaunchKernelGGL(k_commitment_evaluate_jobs, dim3(grid_for(B * n)), dim3(kBlock), 0, st, rows, degree, xs, n, B, out, status);
}
void launch_g1_equal(hipStream_t st, const uint8_t* a, const uint8_t* st_a, const uint8_t* b, const uint8_t* st_b, size_t per_job, size_t B,
                     uint8_t* ok) {
  if (B) hipLaunchKernelGGL(k_g1_equal, dim3(grid_for(B)), dim3(kBlock), 0, st, a, st_a, b, st_b, per_job, B, ok);
}
void launch_dkg_rlc_scalars(hipStream_t st, const uint8_t* seed32, const uint64_t* xs, const uint8_t* vals_fr, size_t n, size_t degree, size_t B,
                            uint32_t* scalars, uint8_t* valid) {
  const size_t lanes = B * (degree + 2);
  if (lanes) hipLaunchKernelGGL(k_dkg_rlc_scalars, dim3(grid_for(lanes)), dim3(kBlock), 0, st, seed32, xs, vals_fr, n, degree, B, scalars, valid);
}
void launch_dkg_rlc_points(hipStream_t st, const uint8_t* rows, size_t degree, const uint8_t* g1_gen, size_t B, uint8_t* out) {
  const size_t words = B * (degree + 2) * 12;
  if (words) hipLaunchKernelGGL(k_dkg_rlc_points, dim3(grid_for(words)), dim3(kBlock), 0, st, rows, degree, g1_gen, B, out);
}
void launch_g1_is_identity(hipStream_t st, const uint8_t* pts, const uint8_t* status, const uint8_t* valid, size_t B, uint8_t* ok) {
  if (B) hipLaunchKernelGGL(k_g1_is_identity, dim3(grid_for(B)), dim3(kBlock), 0, st, pts, status, valid, B, ok);
}

// ---- DKG finalisation (tc_dkg.h): sums of G1 points and of Fr values over the accepted parts ---------------------------
// where output j finds its term 0: consecutive points, or the first column of a bivariate commitment (row(0)[j] = coefficient (j, 0))
struct SumOffPlain {
  __device__ __forceinline__ size_t operator()(size_t j) const { return j * 96; }
};
struct SumOffColumn0 {
  __device__ __forceinline__ size_t operator()(size_t j) const { return bivar_coeff_pos(j, 0) * 96; }
};
// out[j] = sum_{k < n, included} pts[k * term_stride + off(j)].  `parts` (a power of two, 1 .. 64) adjacent lanes per output,
// so an output never spans two waves; their partial sums meet in log2(parts) rounds of one __shfl_xor exchange of the 42
// limbs + one complete addition, as in k_msm_ladder_g1.  No lane of a live output leaves before the last round; the lanes of
// outputs >= B leave as whole groups (parts divides 64).  member: checked-input mode, member[k * B + j] (else null).
template <class OFF>
__global__ __launch_bounds__(kBlock, TC_WAVES_G1_AUX) void k_g1_sum(const uint8_t* __restrict__ pts, size_t term_stride, size_t n,
                                                                    const uint8_t* __restrict__ mask, const uint8_t* __restrict__ member, size_t B,
                                                                    size_t parts, uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                                                    uint8_t* __restrict__ term_bad) {
  const size_t lp = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t j = lp / parts, g = lp % parts;
  if (j >= B) return;
  bool ok;
  G1Jac r = job_g1_sum_part(pts + OFF()(j), term_stride, mask, member ? member + j : nullptr, B, sum_part(n, g, parts), ok, term_bad);
  int good = ok ? 1 : 0;
  TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
    G1Jac o = r;
    TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) {
      o.x.l[i] = __shfl_xor(r.x.l[i], (int)d, 64);
      o.y.l[i] = __shfl_xor(r.y.l[i], (int)d, 64);
      o.z.l[i] = __shfl_xor(r.z.l[i], (int)d, 64);
    }
    good &= __shfl_xor(good, (int)d, 64);
    r = jac_add(r, o);
  }
  if (g != 0) return;
  g1_encode_uncompressed(good ? jac_to_affine(r) : G1Affine::infinity(), out + j * 96);
  if (status) status[j] = good ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
__global__ __launch_bounds__(kBlock) void k_fr_sum(const uint8_t* __restrict__ vals, size_t term_stride, size_t n, const uint8_t* __restrict__ mask,
                                                   size_t B, uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= B) return;
  const uint8_t st = job_fr_sum(vals + j * 32, term_stride, n, mask, out + j * 32);
  if (status) status[j] = st;
}
// out[p] = coefficient 0 of the polynomial through part p's n samples; a rejected part (accept[p] == 0) is not read: zero, OK
__global__ __launch_bounds__(kBlock) void k_fr_interpolate_at_zero(size_t n, const uint64_t* __restrict__ xs, const uint8_t* __restrict__ vals,
                                                                   const uint8_t* __restrict__ accept, size_t P, uint8_t* __restrict__ out,
                                                                   uint8_t* __restrict__ status) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  if (accept && accept[p] == 0) {
    for (int b = 0; b < 32; b++) out[p * 32 + b] = 0;
    status[p] = TC_JOB_OK;
    return;
  }
  status[p] = job_fr_interpolate_at_zero(n, xs + p * n, vals + p * n * 32, out + p * 32);
}
// the first column of P bivariate commitments as consecutive points: out[p * (degree+1) + i] = commits[p][pos(i, 0)], one
// 8-byte word per lane (checked-input mode: what the membership test and the sum then read)
__global__ __launch_bounds__(kBlock) void k_bivar_column0(const uint8_t* __restrict__ commits, size_t stride, size_t degree, size_t P,
                                                          uint8_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t per = (degree + 1) * 12;
  if (t >= P * per) return;
  const size_t p = t / per, i = (t % per) / 12, w = t % 12;
  reinterpret_cast<uint64_t*>(out)[t] = reinterpret_cast<const uint64_t*>(commits + p * stride + bivar_coeff_pos(i, 0) * 96)[w];
}
// tc_dkg_generate_batch's verdict.  Lane p < P: part_status[p] of an accepted part = INVALID_ENCODING for a bad first-column
// point (point_bad, set by k_g1_sum) or a non-canonical value, DUPLICATE_ENTRY for a repeated abscissa (share_st, may be
// null: an observer); a rejected part is OK.
__global__ __launch_bounds__(kBlock) void k_dkg_part_status(const uint8_t* __restrict__ accept, const uint8_t* __restrict__ point_bad,
                                                            const uint8_t* __restrict__ share_st, size_t P, uint8_t* __restrict__ part_status) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  uint8_t st = TC_JOB_OK;
  if (!accept || accept[p] != 0) {
    if (point_bad[p]) st = TC_JOB_INVALID_ENCODING;
    else if (share_st) st = share_st[p];
  }
  part_status[p] = st;
}
// ... and never a partial key: when an accepted part failed, lane i <= degree writes the identity over out_commit[i] and lane
// degree + 1 zero over the share (either may be null)
__global__ __launch_bounds__(kBlock) void k_dkg_generate_guard(const uint8_t* __restrict__ part_status, size_t P, size_t degree,
                                                               uint8_t* __restrict__ out_commit, uint8_t* __restrict__ out_share) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > degree + 1) return;
  bool failed = false;
  for (size_t p = 0; p < P; p++) failed = failed || part_status[p] != TC_JOB_OK;
  if (!failed) return;
  if (i <= degree) {
    if (out_commit) g1_encode_uncompressed(G1Affine::infinity(), out_commit + i * 96);
  } else if (out_share) {
    for (int b = 0; b < 32; b++) out_share[b] = 0;
  }
}

// lanes per output of k_g1_sum: TC_SUM_PARTS when set (forced), else the smallest power of two that gives the launch one wave
// per SIMD (4 per CU), at most 64 and at most n / 2
size_t g1_sum_parts(size_t B, size_t n, int cus, size_t forced) {
  if (forced) return forced;
  const size_t want = (size_t)(cus > 0 ? cus : 256) * 4 * kBlock;
  size_t parts = 1;
  while (parts < 64 && B * parts < want && parts * 2 * 2 <= n) parts *= 2;
  return parts;
}
void launch_g1_sum(hipStream_t st, bool column0, const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* mask, const uint8_t* member,
                   size_t B, size_t parts, uint8_t* out, uint8_t* status, uint8_t* term_bad) {
  if (!B) return;
  if (parts < 1 || parts > 64 || (parts & (parts - 1))) parts = 1;
  const dim3 grid(grid_for(B * parts));
  if (column0)
    hipLaunchKernelGGL(k_g1_sum<SumOffColumn0>, grid, dim3(kBlock), 0, st, pts, term_stride, n, mask, member, B, parts, out, status, term_bad);
  else
    hipLaunchKernelGGL(k_g1_sum<SumOffPlain>, grid, dim3(kBlock), 0, st, pts, term_stride, n, mask, member, B, parts, out, status, term_bad);
}
void launch_fr_sum(hipStream_t st, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* mask, size_t B, uint8_t* out_fr,
                   uint8_t* status) {
  if (B) hipLaunchKernelGGL(k_fr_sum, dim3(grid_for(B)), dim3(kBlock), 0, st, vals_fr, term_stride, n, mask, B, out_fr, status);
}
void launch_fr_interpolate_at_zero(hipStream_t st, size_t n, const uint64_t* xs, const uint8_t* vals_fr, const uint8_t* accept, size_t P,
                                   uint8_t* out_fr, uint8_t* status) {
  if (P) hipLaunchKernelGGL(k_fr_interpolate_at_zero, dim3(grid_for(P)), dim3(kBlock), 0, st, n, xs, vals_fr, accept, P, out_fr, status);
}
void launch_bivar_column0(hipStream_t st, const uint8_t* commits, size_t stride, size_t degree, size_t P, uint8_t* out) {
  const size_t words = P * (degree + 1) * 12;
  if (words) hipLaunchKernelGGL(k_bivar_column0, dim3(grid_for(words)), dim3(kBlock), 0, st, commits, stride, degree, P, out);
}
void launch_dkg_generate_verdict(hipStream_t st, const uint8_t* accept, const uint8_t* point_bad, const uint8_t* share_st, size_t P, size_t degree,
                                 uint8_t* part_status, uint8_t* out_commit, uint8_t* out_share) {
  if (!P) return;
  hipLaunchKernelGGL(k_dkg_part_status, dim3(grid_for(P)), dim3(kBlock), 0, st, accept, point_bad, share_st, P, part_status);
  hipLaunchKernelGGL(k_dkg_generate_guard, dim3(grid_for(degree + 2)), dim3(kBlock), 0, st, (const uint8_t*)part_status, P, degree, out_commit,
                     out_share);
}

// ---- DKG resharing (tc_dkg.h): the same sums with one public weight per term ------------------------------------------------------
// rec[k] = the validated, recoded form of weight k: once per term, whatever the number of outputs
__global__ __launch_bounds__(kBlock) void k_wsum_recode(const uint8_t* __restrict__ w, size_t n, uint32_t* __restrict__ rec) {
  const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (k < n) wsum_recode_weight(w + k * 32, rec + k * kWsumWeightWords);
}
// out[j] = sum_{k < n, included} w_k pts[k * term_stride + off(j)]: k_g1_sum's lanes, every term through a GLV ladder first.  Same
// lane rules -- `parts` adjacent lanes per group, parts | 64, log2(parts) rounds of __shfl_xor + the complete addition, no lane of
// a live group leaves before the last round, the lanes of groups past the end leave as whole groups, the validity flags travel with
// the sums.  A term costs a ladder, and one wave per output leaves most of the GPU idle at the DKG shapes (68 outputs): so the
// terms of an output may be cut into `slices` ranges (wsum_slice_part), group q = s * B + j summing slice s of output j into
// out[q] with its validity byte in part_ok[q] -- what k_g1_sum then adds up as `slices` terms per output.  slices = 1: group j
// is output j, out and status are the call's.  sel: job_g1_wsum_part's term list (n = its length) or null.  Built for one wave per
// SIMD: a launch is a few hundred waves of ladders whose 8-entry table wants the registers.
template <class OFF>
__global__ __launch_bounds__(kBlock, TC_WAVES_G1) void k_g1_wsum(const uint8_t* __restrict__ pts, size_t term_stride, size_t n,
                                                                 const uint32_t* __restrict__ rec, const uint8_t* __restrict__ mask,
                                                                 const uint8_t* __restrict__ member, size_t B, size_t parts, size_t slices,
                                                                 uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                                                 uint8_t* __restrict__ part_ok, const uint32_t* __restrict__ sel) {
  const size_t lp = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t q = lp / parts, g = lp % parts;
  if (q >= B * slices) return;
  const size_t s = q / B, j = q % B;
  bool ok;
  G1Jac r = job_g1_wsum_part(pts + OFF()(j), term_stride, rec, mask, member ? member + j : nullptr, B, wsum_slice_part(n, s, slices, g, parts), ok,
                             nullptr, sel);
  int good = ok ? 1 : 0;
  TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
    G1Jac o = r;
    TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) {
      o.x.l[i] = __shfl_xor(r.x.l[i], (int)d, 64);
      o.y.l[i] = __shfl_xor(r.y.l[i], (int)d, 64);
      o.z.l[i] = __shfl_xor(r.z.l[i], (int)d, 64);
    }
    good &= __shfl_xor(good, (int)d, 64);
    r = jac_add(r, o);
  }
  if (g != 0) return;
  g1_encode_uncompressed(good ? jac_to_affine(r) : G1Affine::infinity(), out + q * 96);
  if (part_ok) part_ok[q] = good ? 1 : 0;
  else if (status) status[q] = good ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
__global__ __launch_bounds__(kBlock) void k_fr_wsum(const uint8_t* __restrict__ vals, size_t term_stride, size_t n, const uint8_t* __restrict__ w,
                                                    const uint8_t* __restrict__ mask, size_t B, uint8_t* __restrict__ out,
                                                    uint8_t* __restrict__ status) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= B) return;
  const uint8_t st = job_fr_wsum(vals + j * 32, term_stride, n, w, mask, out + j * 32);
  if (status) status[j] = st;
}
// tc_dkg_reshare_batch, what EVERY accepted part is examined for.  Lane p < P: dup[p] (its dealer index repeats an earlier accepted
// part's), point_bad[p] (a first-column point does not decode or, member given -- P x (degree+1) verdicts of the membership test --
// is no member) and const_st[p], the constant check against old_commit.evaluate(dealer_idx[p] + 1); a rejected part is not read.
// Lane P: old_bad[0] = old_commit does not decode (old_member, t_old + 1 verdicts or null: or holds a non-member).
__global__ __launch_bounds__(kBlock, TC_WAVES_G1_AUX) void k_reshare_check(const uint8_t* __restrict__ old_commit, const uint8_t* __restrict__ old_member,
                                                                          size_t t_old, const uint64_t* __restrict__ dealer_idx,
                                                                          const uint8_t* __restrict__ commits, size_t stride, size_t degree,
                                                                          const uint8_t* __restrict__ accept, const uint8_t* __restrict__ member, size_t P,
                                                                          uint8_t* __restrict__ const_st, uint8_t* __restrict__ point_bad,
                                                                          uint8_t* __restrict__ dup, uint8_t* __restrict__ old_bad) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p > P) return;
  if (p == P) {
    bool bad = false;
    for (size_t k = 0; k <= t_old; k++) {
      G1Affine c;
      bad = bad || !g1_decode_uncompressed(old_commit + k * 96, c) || (old_member && old_member[k] == 0);
    }
    old_bad[0] = bad ? 1 : 0;
    return;
  }
  uint8_t cs = TC_JOB_OK, pb = 0, du = 0;
  if (reshare_accepted(accept, p)) {
    du = reshare_is_duplicate(accept, dealer_idx, p) ? 1 : 0;
    for (size_t i = 0; i <= degree; i++) {
      G1Affine c;
      if (!g1_decode_uncompressed(commits + p * stride + bivar_coeff_pos(i, 0) * 96, c) || (member && member[p * (degree + 1) + i] == 0)) pb = 1;
    }
    cs = job_reshare_constant_check(old_commit, t_old, dealer_idx[p], commits + p * stride);
  }
  const_st[p] = cs;
  point_bad[p] = pb;
  dup[p] = du;
}
// part_status[p], the first matching code: INVALID_ENCODING (a bad first-column point, a non-canonical value), DUPLICATE_ENTRY (a
// repeated dealer index, a repeated abscissa), SHARE_MISMATCH; a rejected part, and every part under a bad old_commit, is OK
__global__ __launch_bounds__(kBlock) void k_reshare_part_status(const uint8_t* __restrict__ accept, const uint8_t* __restrict__ const_st,
                                                                const uint8_t* __restrict__ point_bad, const uint8_t* __restrict__ dup,
                                                                const uint8_t* __restrict__ share_st, const uint8_t* __restrict__ old_bad, size_t P,
                                                                uint8_t* __restrict__ part_status) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  uint8_t st = TC_JOB_OK;
  if (old_bad[0] == 0 && reshare_accepted(accept, p)) {
    const uint8_t ss = share_st ? share_st[p] : (uint8_t)TC_JOB_OK;
    if (point_bad[p] || const_st[p] == TC_JOB_INVALID_ENCODING || ss == TC_JOB_INVALID_ENCODING) st = TC_JOB_INVALID_ENCODING;
    else if (dup[p] || ss == TC_JOB_DUPLICATE_ENTRY) st = TC_JOB_DUPLICATE_ENTRY;
    else if (const_st[p] == TC_JOB_SHARE_MISMATCH) st = TC_JOB_SHARE_MISMATCH;
  }
  part_status[p] = st;
}
// the verdict and the plan, ONE lane: status[0]; used[p] (zero unless the verdict is OK); the dealers of S and their Lagrange
// coefficients at zero (lagrange_all_at_zero over distinct abscissae: duplicates were turned away above), written as weight p of
// `weights` (P x 32 B, zeroed by the caller) for the parts of S.  sel_idx / sel_part: t_old + 1 entries, lam: (t_old + 1) x 8 words,
// ws: 4 (t_old + 1) x 8 words.
__global__ __launch_bounds__(kBlock) void k_reshare_plan(const uint8_t* __restrict__ accept, const uint64_t* __restrict__ dealer_idx, size_t t_old, size_t P,
                                                         const uint8_t* __restrict__ part_status, const uint8_t* __restrict__ old_bad,
                                                         uint8_t* __restrict__ used, uint32_t* __restrict__ sel_part, uint64_t* __restrict__ sel_idx,
                                                         uint32_t* __restrict__ lam, uint32_t* __restrict__ ws, uint8_t* __restrict__ weights,
                                                         uint8_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint8_t st = old_bad[0] ? (uint8_t)TC_JOB_INVALID_ENCODING : (uint8_t)TC_JOB_OK;
  for (size_t p = 0; p < P && st == TC_JOB_OK; p++) st = part_status[p];
  bool selected = false;
  if (st == TC_JOB_OK) {
    selected = reshare_select(accept, dealer_idx, t_old, P, used, sel_part, sel_idx, nullptr);
    if (!selected) st = TC_JOB_NOT_ENOUGH_SHARES;
  }
  if (selected) {
    st = lagrange_all_at_zero(sel_idx, (int)t_old, lam, ws);
    if (st == TC_JOB_OK) {
      for (size_t i = 0; i <= t_old; i++)
        for (int b = 0; b < 32; b++) weights[(size_t)sel_part[i] * 32 + b] = (uint8_t)(lam[i * 8 + (b >> 2)] >> (8 * (b & 3)));
    }
  }
  if (st != TC_JOB_OK)
    for (size_t p = 0; p < P; p++) used[p] = 0;
  status[0] = st;
}
// ... and never a partial key: unless the verdict is OK, lane i <= degree writes the identity over out_commit[i] and lane degree + 1
// zero over the share (either may be null)
__global__ __launch_bounds__(kBlock) void k_reshare_guard(const uint8_t* __restrict__ status, size_t degree, uint8_t* __restrict__ out_commit,
                                                          uint8_t* __restrict__ out_share) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > degree + 1 || status[0] == TC_JOB_OK) return;
  if (i <= degree) {
    if (out_commit) g1_encode_uncompressed(G1Affine::infinity(), out_commit + i * 96);
  } else if (out_share) {
    for (int b = 0; b < 32; b++) out_share[b] = 0;
  }
}

// lanes per output of k_g1_wsum: TC_SUM_PARTS when set (forced), else g1_sum_parts' rule with the cap at n instead of n / 2 -- a
// term costs a ladder here, so a lane with ONE term is still work worth a lane
size_t g1_wsum_parts(size_t B, size_t n, int cus, size_t forced) {
  if (forced) return forced;
  const size_t want = (size_t)(cus > 0 ? cus : 256) * 4 * kBlock;
  size_t parts = 1;
  while (parts < 64 && B * parts < want && parts * 2 <= n) parts *= 2;
  return parts;
}
// slices per output: TC_WSUM_SLICES when set (forced), else, once an output has a whole wave and still more than one term per
// lane, as many as bring it to one term per lane -- while the launch stays within one wave per SIMD (4 per CU)
size_t g1_wsum_slices(size_t B, size_t n, size_t parts, int cus, size_t forced) {
  size_t slices = forced;
  if (!slices) {
    if (parts < 64 || n <= 64) return 1;
    const size_t room = (size_t)(cus > 0 ? cus : 256) * 4 / (B ? B : 1);
    slices = (n + 63) / 64;
    if (slices > room) slices = room;
  }
  if (slices > n) slices = n;
  return slices < 1 ? 1 : slices;
}
size_t wsum_rec_words() { return kWsumWeightWords; }
void launch_wsum_recode(hipStream_t st, const uint8_t* weights_fr, size_t n, uint32_t* rec) {
  if (n) hipLaunchKernelGGL(k_wsum_recode, dim3(grid_for(n)), dim3(kBlock), 0, st, weights_fr, n, rec);
}
void launch_g1_wsum(hipStream_t st, bool column0, const uint8_t* pts, size_t term_stride, size_t n, const uint32_t* rec, const uint8_t* mask,
                    const uint8_t* member, size_t B, size_t parts, size_t slices, uint8_t* out, uint8_t* status, uint8_t* part_ok,
                    const uint32_t* sel) {
  if (!B) return;
  if (parts < 1 || parts > 64 || (parts & (parts - 1))) parts = 1;
  if (slices < 1 || !part_ok) slices = 1;
  if (slices == 1) part_ok = nullptr;
  const dim3 grid(grid_for(B * slices * parts));
  if (column0)
    hipLaunchKernelGGL(k_g1_wsum<SumOffColumn0>, grid, dim3(kBlock), 0, st, pts, term_stride, n, rec, mask, member, B, parts, slices, out, status,
                       part_ok, sel);
  else
    hipLaunchKernelGGL(k_g1_wsum<SumOffPlain>, grid, dim3(kBlock), 0, st, pts, term_stride, n, rec, mask, member, B, parts, slices, out, status,
                       part_ok, sel);
}
void launch_fr_wsum(hipStream_t st, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* weights_fr, const uint8_t* mask, size_t B,
                    uint8_t* out_fr, uint8_t* status) {
  if (B) hipLaunchKernelGGL(k_fr_wsum, dim3(grid_for(B)), dim3(kBlock), 0, st, vals_fr, term_stride, n, weights_fr, mask, B, out_fr, status);
}
void launch_reshare_check(hipStream_t st, const uint8_t* old_commit, const uint8_t* old_member, size_t t_old, const uint64_t* dealer_idx,
                          const uint8_t* commits, size_t stride, size_t degree, const uint8_t* accept, const uint8_t* member, size_t P,
                          uint8_t* const_st, uint8_t* point_bad, uint8_t* dup, uint8_t* old_bad) {
  hipLaunchKernelGGL(k_reshare_check, dim3(grid_for(P + 1)), dim3(kBlock), 0, st, old_commit, old_member, t_old, dealer_idx, commits, stride, degree,
                     accept, member, P, const_st, point_bad, dup, old_bad);
}
size_t reshare_plan_ws_words(size_t t_old) { return 5 * (t_old + 1) * 8; }  // lam, then lagrange_all_at_zero's scratch
void launch_reshare_verdict(hipStream_t st, const uint8_t* accept, const uint64_t* dealer_idx, size_t t_old, size_t P, const uint8_t* const_st,
                            const uint8_t* point_bad, const uint8_t* dup, const uint8_t* share_st, const uint8_t* old_bad, uint8_t* part_status,
                            uint8_t* used, uint32_t* sel_part, uint64_t* sel_idx, uint32_t* ws, uint8_t* weights, uint8_t* status) {
  if (!P) return;
  hipLaunchKernelGGL(k_reshare_part_status, dim3(grid_for(P)), dim3(kBlock), 0, st, accept, const_st, point_bad, dup, share_st, old_bad, P, part_status);
  hipLaunchKernelGGL(k_reshare_plan, dim3(1), dim3(kBlock), 0, st, accept, dealer_idx, t_old, P, (const uint8_t*)part_status, old_bad, used, sel_part,
                     sel_idx, ws, ws + (t_old + 1) * 8, weights, status);
}
void launch_reshare_guard(hipStream_t st, const uint8_t* status, size_t degree, uint8_t* out_commit, uint8_t* out_share) {
  hipLaunchKernelGGL(k_reshare_guard, dim3(grid_for(degree + 2)), dim3(kBlock), 0, st, status, degree, out_commit, out_share);
}

}  // namespace tc
