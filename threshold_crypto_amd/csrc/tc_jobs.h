// Per-lane job bodies: one independent (message, share-set) job or one curve op per lane.
// The __global__ kernels in tc_kernels.hip call these with the lane's slice of the batch;
// tests/hostsim calls the same bodies from a host loop (test harness only).
#pragma once
#include "tc_codec.h"
#include "tc_gls.h"
#include "tc_hash.h"
#include "tc_pairing.h"
#include "tc_robust.h"
#include "tc_threshold.h"

namespace tc {

template <class F>
struct PointIO;

// lanes that work on one job: Fq2 jobs are spread over a lane pair in the hipcc build (tc_common.h)
template <class F>
struct JobLanes {
  static constexpr int N = 1;
};
template <>
struct JobLanes<Fq2> {
  static constexpr int N = kG2Lanes;
};

template <>
struct PointIO<Fq> {
  static constexpr int BYTES = 96;
  static constexpr int CBYTES = 48;
  TC_HD static bool decode(const uint8_t* b, Affine<Fq>& p) { return g1_decode_uncompressed(b, p); }
  TC_HD static void encode(const Affine<Fq>& p, uint8_t* b) { g1_encode_uncompressed(p, b); }
};
template <>
struct PointIO<Fq2> {
  static constexpr int BYTES = 192;
  static constexpr int CBYTES = 96;
  TC_HD static bool decode(const uint8_t* b, Affine<Fq2>& p) { return g2_decode_uncompressed(b, p); }
  TC_HD static void encode(const Affine<Fq2>& p, uint8_t* b) { g2_encode_uncompressed(p, b); }
};

// [k] p.  G1: 2-dimensional GLV through phi (128 doublings); G2: 4-dimensional GLS through psi
// (64 doublings) -- tc_gls.h -- instead of the reference's 255-bit ladder.  Operands must lie in
// the prime-order subgroup, as every G1/G2 value the reference holds does.
TC_HD Jac<Fq> point_mul_scalar(const Affine<Fq>& p, const uint32_t* k) { return g1_mul_glv(p, k); }
TC_HD Jac<Fq> point_mul_scalar(const Jac<Fq>& p, const uint32_t* k) { return g1_mul_glv(p, k); }
TC_HD Jac<Fq2> point_mul_scalar(const Jac<Fq2>& p, const uint32_t* k) { return g2_mul_gls(p, k); }
TC_HD Jac<Fq2> point_mul_scalar(const Affine<Fq2>& p, const uint32_t* k) {
  return g2_mul_gls(p, k);
}

// order-r membership (tc_sqrt.h: Scott's endomorphism tests, one / two 64-bit ladders)
TC_HD bool point_in_subgroup(const Affine<Fq>& p) { return g1_in_subgroup(p); }
TC_HD bool point_in_subgroup(const Affine<Fq2>& p) { return g2_in_subgroup(p); }

// out = fr * pt           (CurveAffine::mul: sign_g2 src/lib.rs:373, decrypt_share :461)
// The scalar is shared by all lanes of a wave (one secret key share per wave), so the
// bit-serial double-and-add below has wave-uniform control flow.
template <class F>
TC_HD uint8_t job_point_mul(const uint8_t* fr_le32, const uint8_t* pt, uint8_t* out) {
  uint32_t k[8];
  Affine<F> p;
  bool ok = fr_from_le32(fr_le32, k);
  ok &= PointIO<F>::decode(pt, p);
  if (!ok) {
    PointIO<F>::encode(Affine<F>::infinity(), out);
    return TC_JOB_INVALID_ENCODING;
  }
  PointIO<F>::encode(jac_to_affine(point_mul_scalar(p, k)), out);
  return TC_JOB_OK;
}

// the G1 multiplication with its ladder table in the wave's arena slot (tc_gls.h g1_mul_glv_arena): the body of the kernel built
// for two waves per SIMD.  Every lane of the wave runs the ladder (a failed decode multiplies the identity's stand-in).
TC_HD uint8_t job_g1_mul_arena(const uint8_t* fr_le32, const uint8_t* pt, uint8_t* out) {
  uint32_t k[8];
  G1Affine p;
  bool ok = fr_from_le32(fr_le32, k);
  ok &= g1_decode_uncompressed(pt, p);
  if (!ok) {
    p = G1Affine{g1_generator().x, g1_generator().y, true};
    TC_UNROLL for (int i = 0; i < 8; i++) k[i] = (i == 0) ? 1u : 0u;
  }
  const G1Affine r = jac_to_affine(g1_mul_glv_arena(p, k));
  g1_encode_uncompressed(ok ? r : G1Affine::infinity(), out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// out[s] = fr[s] * pt for n <= C scalars and ONE G2 point (the S signers of tc_g2_mul_batch over the
// same hash point): one decode, one table of psi-images (tc_gls.h g2_sac_table) and one inversion
// for the n results.  A bad point fails all n outputs, a bad scalar only its own.
constexpr int kMulShare = 4;
TC_HD void job_g2_mul_shared(const uint8_t* fr_le32, int n, const uint8_t* pt, uint8_t* out, uint8_t* status, bool leader) {
  G2Affine p;
  const bool pok = g2_decode_uncompressed(pt, p);
  if (!pok) p = G2Affine::infinity();
  G2Affine base[4];
  g2_gls_bases(p, base);
  G2SacTable tb;
  g2_sac_table_call(base, tb);
  G2Jac res[kMulShare];
  bool ok[kMulShare];
  TC_NOUNROLL for (int s = 0; s < n; s++) {
    uint32_t k[8];
    ok[s] = fr_from_le32(fr_le32 + 32 * s, k) && pok;
    uint64_t d[4];
    const bool flip = gls_decompose_odd(k, d);
    G2Jac r = g2_sac_ladder_call(tb, d);
    r.y = Fq2::select(flip, -r.y, r.y);
    res[s] = G2Jac::select(ok[s], r, G2Jac::infinity());
  }
  G2Affine aff[kMulShare];
  jac_batch_to_affine<Fq2, kMulShare>(res, aff, n);
  TC_NOUNROLL for (int s = 0; s < n; s++) {
    g2_encode_uncompressed(aff[s], out + (size_t)s * 192);
    if (status && leader) status[s] = ok[s] ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  }
}

constexpr int kGatherShare = 8;  // scalars per table in the gather kernel (68 signers: 9 tables per message instead of 17)
// out[s] = sk[idx[s]] * pt for n <= kGatherShare signer indices into a table of N secret key shares: the shares of
// ONE message by the signers of its subset (SecretKeyShare::sign_g2, src/lib.rs:442-444, for every selected
// signer), generated on the device so that a (t, N, batch) workload needs only the key set and the hash points.
// An index >= N fails its own output.
TC_HD void job_g2_mul_gather(const uint8_t* sk_table, size_t N, const uint64_t* idx, int n, const uint8_t* pt, uint8_t* out,
                             uint8_t* status, bool leader) {
  G2Affine p;
  const bool pok = g2_decode_uncompressed(pt, p);
  if (!pok) p = G2Affine::infinity();
  G2Affine base[4];
  g2_gls_bases(p, base);
  G2SacTable tb;
  g2_sac_table_call(base, tb);
  G2Jac res[kGatherShare];
  bool ok[kGatherShare];
  TC_NOUNROLL for (int s = 0; s < n; s++) {
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t i = idx[s];
    ok[s] = pok && i < N;
    if (i < N) ok[s] = fr_from_le32(sk_table + 32 * i, k) && ok[s];
    uint64_t d[4];
    const bool flip = gls_decompose_odd(k, d);
    G2Jac r = g2_sac_ladder_call(tb, d);
    r.y = Fq2::select(flip, -r.y, r.y);
    res[s] = G2Jac::select(ok[s], r, G2Jac::infinity());
  }
  G2Affine aff[kGatherShare];
  jac_batch_to_affine<Fq2, kGatherShare>(res, aff, n);
  TC_NOUNROLL for (int s = 0; s < n; s++) {
    g2_encode_uncompressed(aff[s], out + (size_t)s * 192);
    if (status && leader) status[s] = ok[s] ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  }
}

// k * c mod r for c = FR_COFACTOR_FIX (canonical words in and out)
TC_HD void fr_mul_cofactor_fix(const uint32_t* k, uint32_t* out) {
  (Fr::from_canonical(k) * Fr::from_canonical(FR_COFACTOR_FIX)).to_canonical(out);
}
// scalar of a signer folded with the hash's constant: out = fr * c mod r; a non-canonical scalar stays
// non-canonical (all ones) so that the multiplication kernel flags it as before
TC_HD void job_fr_scale_cofactor_fix(const uint8_t* fr_le32, uint8_t* out_le32) {
  uint32_t k[8], kc[8];
  const bool ok = fr_from_le32(fr_le32, k);
  fr_mul_cofactor_fix(k, kc);
  TC_UNROLL for (int i = 0; i < 8; i++) {
    const uint32_t w = ok ? kc[i] : 0xffffffffu;
    out_le32[4 * i] = (uint8_t)w;
    out_le32[4 * i + 1] = (uint8_t)(w >> 8);
    out_le32[4 * i + 2] = (uint8_t)(w >> 16);
    out_le32[4 * i + 3] = (uint8_t)(w >> 24);
  }
}
// G1 operand of a pairing against a hash point, folded with the hash's constant: out = [c] P.
// An encoding that does not decode is passed through unchanged, so the pairing kernel rejects it
// exactly as it would have rejected the original.
TC_HD void job_g1_scale_cofactor_fix(const uint8_t* in96, uint8_t* out96) {
  G1Affine p;
  if (!g1_decode_uncompressed(in96, p)) {
    for (int i = 0; i < 96; i++) out96[i] = in96[i];
    return;
  }
  g1_encode_uncompressed(jac_to_affine(g1_mul_glv(p, FR_COFACTOR_FIX)), out96);
}

// Lagrange coefficient (job, position i) -> 8 canonical LE words
TC_HD uint8_t job_lagrange(const uint64_t* idx, int t, int i, uint32_t* out_words) {
  Fr lam;
  if (!lagrange_coeff_at_zero(idx, t, i, lam)) {
    for (int w = 0; w < 8; w++) out_words[w] = 0;
    return TC_JOB_DUPLICATE_ENTRY;
  }
  lam.to_canonical(out_words);
  return TC_JOB_OK;
}

// out = sum_{i < n} scalar_i * point_i   (scalars: n x 8 canonical LE words, < r)
// Used by interpolate (below) and by Commitment::evaluate (src/poly.rs:497-508), which is the
// linear combination sum_k x^k * commit[k].
template <class F>
TC_HD uint8_t job_lincomb(int n, const uint8_t* points, const uint32_t* scalars, uint8_t* out) {
  constexpr int PB = PointIO<F>::BYTES;
  Jac<F> total = Jac<F>::infinity();
  bool ok = true;
  TC_NOUNROLL for (int base = 0; base < n; base += 4) {
    const int k = (n - base) < 4 ? (n - base) : 4;
    Affine<F> pts[4];
    uint32_t sc[4][8];
    TC_NOUNROLL for (int j = 0; j < 4; j++) {
      if (j < k) {
        ok &= PointIO<F>::decode(points + (size_t)(base + j) * PB, pts[j]);
        for (int w = 0; w < 8; w++) sc[j][w] = scalars[(size_t)(base + j) * 8 + w];
        ok &= limbs_lt_p<FrParams>(sc[j]);
      } else {
        pts[j] = Affine<F>::infinity();
        for (int w = 0; w < 8; w++) sc[j][w] = 0;
      }
    }
    Jac<F> part = lincomb_chunk4(pts, sc);
    total = jac_add(total, part);
  }
  if (!ok) {
    PointIO<F>::encode(Affine<F>::infinity(), out);
    return TC_JOB_INVALID_ENCODING;
  }
  PointIO<F>::encode(jac_to_affine(total), out);
  return TC_JOB_OK;
}

// Classes of the common denominator D of the small-index fast path (below).  The last step of that
// path is [1/D] Q, in general one full GLS multiplication; two classes are much cheaper, and the
// combine kernels group jobs by class so that a wave takes ONE of the branches (k_combine.hip):
//   D = 1            nothing to do
//   D = 2^a, a <= 16 |x| = 2^16 * 0xd20100000001 and x^2 - x^4 = 1 (mod r), so on G2
//                    [1/D] Q = [|x| / D] (psi^3(Q) - psi(Q)):  16 - a doublings, then the 48-bit ladder of
//                    |x| >> 16 (Hamming weight 6): 62 doublings + 5 additions instead of 64 + 64 + a table
constexpr int kCombineClassGeneric = 0, kCombineClassOne = 1, kCombineClassPow2 = 2, kCombineClasses = 3;
TC_HD int combine_denominator_class(uint64_t d_abs) {
  if (d_abs == 1) return kCombineClassOne;
  if ((d_abs & (d_abs - 1)) == 0 && d_abs <= (1ull << 16)) return kCombineClassPow2;
  return kCombineClassGeneric;
}
// [sign / d_abs] q
TC_HD G1Jac combine_divide(const G1Jac& q, uint64_t d_abs, bool d_neg) {
  uint32_t dinv[8];
  fr_inverse_of_small(d_abs, d_neg, dinv);
  return point_mul_scalar(q, dinv);
}
// the same with the ladder's table in the lane's arena entries (the two-waves-per-SIMD build of k_combine_fast<Fq>)
TC_HD G1Jac combine_divide_arena(const G1Jac& q, uint64_t d_abs, bool d_neg) {
  // a wave whose jobs all have D = 1 (the combine kernels group jobs by class from kG1GroupMinJobs on) has nothing to divide by;
  // G1 has no cheap form for D = 2^a (the G2 shortcut rests on psi = [x])
  if (!wave_any(d_abs != 1)) {
    G1Jac r = q;
    r.y = Fq::select(d_neg, -r.y, r.y);
    return r;
  }
  uint32_t dinv[8];
  fr_inverse_of_small(d_abs, d_neg, dinv);
  G1Jac r = g1_mul_glv_arena(G1Affine{q.x, q.y, q.is_inf()}, dinv);
  r.z = coord_norm(r.z * q.z);
  return r;
}

TC_HD G2Jac combine_divide(const G2Jac& q, uint64_t d_abs, bool d_neg) {
  const int cls = combine_denominator_class(d_abs);
  G2Jac r = q;
  if (wave_any(cls == kCombineClassGeneric)) {
    uint32_t dinv[8];
    fr_inverse_of_small(d_abs, false, dinv);
    r = G2Jac::select(cls == kCombineClassGeneric, point_mul_scalar(q, dinv), r);
  }
  if (wave_any(cls == kCombineClassPow2)) {
    const G2Jac p1 = g2_psi(q);
    const G2Jac p3 = g2_psi(g2_psi(p1));
    G2Jac base = jac_add(p3, jac_neg(p1));  // psi^3(Q) - psi(Q)
    const int pre = 16 - (int)__builtin_ctzll(d_abs | (1ull << 16));  // 16 - a doublings first
    TC_NOUNROLL for (int i = 0; i < 15; i++) base = G2Jac::select(i < pre, jac_dbl(base), base);
    const uint64_t s = BLS_X_ABS >> 16;
    const G2Affine ba{base.x, base.y, base.is_inf()};  // affine on the curve scaled by base.z (tc_gls.h)
    G2Jac acc = jac_ladder_uniform(ba, s, 47);  // bit 47 is the leading one
    acc.z = coord_norm(acc.z * base.z);
    r = G2Jac::select(cls == kCombineClassPow2, acc, r);
  }
  r.y = Fq2::select(d_neg, -r.y, r.y);
  return r;
}
TC_HD G2Jac combine_divide_arena(const G2Jac& q, uint64_t d_abs, bool d_neg) { return combine_divide(q, d_abs, d_neg); }  // (G2: always in the arena)
TC_HD_NOINLINE G2Jac combine_divide_call(const G2Jac& q, uint64_t d_abs, bool d_neg) { return combine_divide(q, d_abs, d_neg); }
// [1 / d_abs] q for a WAVE-UNIFORM denominator of the generic class (a wave of jobs over one signer subset): D^-1 mod r is
// the wave's, so its base-|x| digits steer the width-4 NAF ladder of tc_gls.h (no odd first digit needed: no flip).
// exc: the lane may have met a special case of the addition and its result is to be recomputed by combine_divide.
TC_HD_NOINLINE G2Jac combine_divide_uniform(const G2Jac& q, uint64_t d_abs, bool& exc) {
  uint32_t dinv[8];
  fr_inverse_of_small(d_abs, false, dinv);
  uint64_t d[4];
  gls_decompose(dinv, d);
  TC_UNROLL for (int j = 0; j < 4; j++) d[j] = wave_uniform(d[j]);
  G2WnafTable t;
  exc = exc || q.is_inf();
  g2_wnaf_table(q, t, exc);
  return g2_wnaf_ladder(t, d, exc);
}

// The same through the quotient of |x| by D (tc_gls.h combine_quotient_decompose): one ladder over q = |x| / D on a point
// made from coefficients as short as D.  d_abs must be one the decomposition takes (combine_divide_takes_quotient).
// (This entry, combine_divide_quotient_macs and combine_divide_takes_quotient keep the chain of m = 0, width 3 for the conformance
// suite, which pins it digit by digit; no kernel calls them: a wave runs combine_divide_cheapest below.)
TC_HD_NOINLINE G2Jac combine_divide_quotient(const G2Jac& q, uint64_t d_abs, bool& exc) {
  uint64_t qq = 0;
  int64_t T[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
  // (decomposed on EVERY lane, before the lane's own flags are looked at: the wave takes q, T and E from its first lane, and a
  // first lane with q at infinity that skipped the decomposition handed zeros to all 32 jobs, which then all raised exc)
  const bool taken = combine_quotient_decompose(d_abs, &qq, T, E);
  exc = exc || q.is_inf() || !taken;
  TC_UNROLL for (int j = 0; j < 4; j++) {
    T[j] = (int64_t)wave_uniform((uint64_t)T[j]);
    E[j] = (int64_t)wave_uniform((uint64_t)E[j]);
  }
  return g2_quotient_mul(q, wave_uniform(qq), T, E, exc);
}
// Which of the two forms a wave takes: the multiply-adds of both, predicted from the digits -- the doublings and the
// additions of each ladder times what a doubling and a mixed addition execute (two lanes, tests/count_ops.py), plus what
// each form executes besides (the tables, the common Z, the bases).  The quotient form wins for every D below 2^13 or so
// and loses from 2^16 on, where T and E are as long as a fifth of q.
constexpr uint32_t kMacsDbl = 6272, kMacsAdd = 11368, kMacsPsi2 = 784, kMacsUniformFixed = 91938, kMacsQuotientFixed = 39410;
TC_HD uint32_t combine_divide_uniform_macs(uint64_t d_abs) {
  uint32_t dinv[8];
  fr_inverse_of_small(d_abs, false, dinv);
  uint64_t d[4];
  gls_decompose(dinv, d);
  int top = 0, nz = 0, nz2 = 0;  // nz2: look-ups that take psi^2 of an entry
  // (the weight and the top column of each digit's width-4 NAF, tc_gls.h wnaf_shape: the digits themselves are not needed here)
  TC_NOUNROLL for (int j = 0; j < 4; j++) {
    int n = 0, t = 0;
    wnaf_shape<4>(d[j], &n, &t);
    nz += n;
    nz2 += (j >> 1) * n;
    if (t > top) top = t;
  }
  return kMacsUniformFixed + (uint32_t)top * kMacsDbl + (uint32_t)(nz - 1) * kMacsAdd + (uint32_t)nz2 * kMacsPsi2;
}
TC_HD uint32_t combine_divide_quotient_macs(uint64_t q, const int64_t* T, const int64_t* E) {
  const QuotNaf nt = quot_naf(T), ne = quot_naf(E);
  int8_t dig[kWnafCols];
  wnaf_recode<kQuotWidth>(q, dig);
  int top = ne.any() ? 63 - (int)__builtin_clzll(ne.any()) : 0, nz = 0, nz2 = 0;
  TC_NOUNROLL for (int col = 0; col < kWnafCols; col++)
    if (dig[col]) {
      nz++;
      if (col > top) top = col;
    }
  TC_UNROLL for (int j = 0; j < 4; j++) {
    const int n = __builtin_popcountll(nt.pos[j] | nt.neg[j]) + __builtin_popcountll(ne.pos[j] | ne.neg[j]);
    nz += n;
    nz2 += (j >> 1) * n;
  }
  top += nt.any() ? 63 - (int)__builtin_clzll(nt.any()) : 0;
  return kMacsQuotientFixed + (uint32_t)top * kMacsDbl + (uint32_t)(nz - 2) * kMacsAdd + (uint32_t)nz2 * kMacsPsi2;
}
// The digits of the quotient form are free in two ways: for any integer m
//     D^-1 = sum_j (T_j (q + m) + (E_j - m T_j)) psi^j  (mod r),
// so the ladder may run over q + m with E' = E - m T, and any NAF width may recode q + m.  The plan is the cheapest of
// m in {0, 1} -- the two integers next to |x| / D: m = 1 rounds it up, and E' is about a bit shorter when |x| mod D > D / 2; any
// other m moves q + m away from |x| / D and lengthens E' by |m T| -- x width in {2, 3, 4} (the odd multiples of width 4 and the
// two bases fill 6 of the 8 entries of the lane pair's arena table) by the multiply-adds g2_quotient_mul_width executes, counted
// as combine_divide_quotient_macs counts them: what the widths execute besides the doublings and additions (P1 alone; P1, 3 P1;
// P1 .. 7 P1 on a common Z) is kMacsQuotientFixedOf[width - 2].  Ties go to m = 0, width 3, the chain before the plan.
// q + m >= q >= 3 and |E'_j| <= D + 2 < 2^63 stay inside what the ladder accepts.  A function of (q, T, E) alone: wave-uniform,
// scalar work, one loop step per nonzero digit of the four width-3 and width-4 candidates (DESIGN 4.12 has the count).
constexpr int kQuotPlanShiftLo = 0, kQuotPlanShiftHi = 1;
static_assert(kQuotPlanShiftLo == 0, "combine_quotient_plan starts from E and q themselves");
constexpr uint32_t kMacsQuotientFixedOf[3] = {15890, kMacsQuotientFixed, 85666};
struct QuotPlan {
  int m, width;
  uint32_t macs;
};
// the additions and psi^2 look-ups of the NAFs of four coefficients of psi^j, and their top column
struct QuotCoeffCost {
  uint32_t macs;
  int top;
};
TC_HD QuotCoeffCost quot_coeff_cost(const int64_t* c) {
  uint64_t any = 0;
  int nz = 0, nz2 = 0;
  TC_UNROLL for (int j = 0; j < 4; j++) {
    const uint64_t cols = naf_columns(c[j]);
    const int n = __builtin_popcountll(cols);
    any |= cols;
    nz += n;
    nz2 += (j >> 1) * n;
  }
  return QuotCoeffCost{(uint32_t)nz * kMacsAdd + (uint32_t)nz2 * kMacsPsi2, any ? 63 - (int)__builtin_clzll(any) : 0};
}
// the ladder of q at width W beside E digits that reach column top_e: the table, the doublings, the additions of q's digits
template <int W>
TC_HD uint32_t quot_ladder_macs(uint64_t q, int top_e) {
  int nz, top;
  wnaf_shape<W>(q, &nz, &top);
  if (top < top_e) top = top_e;
  return kMacsQuotientFixedOf[W - 2] + (uint32_t)top * kMacsDbl + (uint32_t)nz * kMacsAdd;
}
// one candidate, whatever m and width (the host tests force candidates the planner does not look at)
TC_HD uint32_t combine_quotient_candidate_macs(uint64_t q, const int64_t* T, const int64_t* E, int m, int width) {
  int64_t Em[4];
  TC_UNROLL for (int j = 0; j < 4; j++) Em[j] = E[j] - (int64_t)m * T[j];
  const QuotCoeffCost ct = quot_coeff_cost(T), ce = quot_coeff_cost(Em);
  const uint64_t qm = q + (uint64_t)(int64_t)m;
  const uint32_t ladder = width == 2 ? quot_ladder_macs<2>(qm, ce.top) : width == 3 ? quot_ladder_macs<3>(qm, ce.top) : quot_ladder_macs<4>(qm, ce.top);
  return (uint32_t)ct.top * kMacsDbl + ct.macs - 2 * kMacsAdd + ce.macs + ladder;
}
#if !defined(__HIPCC__)
inline int g_tc_force_quot_plan = 0;  // host test build: 16 (m + 8) + width = that plan, whatever it costs; 0 = the cheapest
#endif
TC_HD QuotPlan combine_quotient_plan(uint64_t q, const int64_t* T, const int64_t* E) {
#if !defined(__HIPCC__)
  if (g_tc_force_quot_plan) {
    const int m = g_tc_force_quot_plan / 16 - 8, width = g_tc_force_quot_plan % 16;
    return QuotPlan{m, width, combine_quotient_candidate_macs(q, T, E, m, width)};
  }
#endif
  // what no candidate changes: the ladder of P1 = T(psi) P
  const QuotCoeffCost ct = quot_coeff_cost(T);
  const uint32_t base = (uint32_t)ct.top * kMacsDbl + ct.macs - 2 * kMacsAdd;
  QuotPlan best{0, kQuotWidth, 0xffffffffu};
  int64_t Em[4] = {E[0], E[1], E[2], E[3]};
  // (m = 0 first, then width 3 first: a later candidate replaces the plan only when it is strictly cheaper)
  TC_UNROLL for (int m = kQuotPlanShiftLo; m <= kQuotPlanShiftHi; m++) {
    const QuotCoeffCost ce = quot_coeff_cost(Em);
    const uint64_t qm = q + (uint64_t)m;
    const uint32_t fixed_m = base + ce.macs;
    const uint32_t w3 = fixed_m + quot_ladder_macs<3>(qm, ce.top), w2 = fixed_m + quot_ladder_macs<2>(qm, ce.top), w4 = fixed_m + quot_ladder_macs<4>(qm, ce.top);
    if (w3 < best.macs) best = QuotPlan{m, 3, w3};
    if (w2 < best.macs) best = QuotPlan{m, 2, w2};
    if (w4 < best.macs) best = QuotPlan{m, 4, w4};
    TC_UNROLL for (int j = 0; j < 4; j++) Em[j] -= T[j];
  }
  return best;
}
// The planned form of the division (combine_divide_quotient below keeps the chain of m = 0, width 3): the ladder over q + m at
// the planned width, for the wave-uniform q, T, E of a wave-uniform denominator.
TC_HD G2Jac combine_divide_planned(const G2Jac& a, uint64_t q, const int64_t* T, const int64_t* E, const QuotPlan& plan, bool& exc) {
  int64_t Tu[4], Eu[4];
  TC_UNROLL for (int j = 0; j < 4; j++) {
    Tu[j] = (int64_t)wave_uniform((uint64_t)T[j]);
    Eu[j] = (int64_t)wave_uniform((uint64_t)(E[j] - (int64_t)plan.m * T[j]));
  }
  const int width = (int)wave_uniform((uint64_t)plan.width);
  exc = exc || a.is_inf();
  return g2_quotient_mul_width(a, wave_uniform(q + (uint64_t)(int64_t)plan.m), Tu, Eu, width, exc);
}
#if !defined(__HIPCC__)
inline int g_tc_force_divide_form = 0;  // host test build: 1 = the 4-dimensional ladder, 2 = the quotient form wherever it exists
#endif
// [1 / d_abs] a for a wave-uniform d_abs of the generic class by the cheaper of the planned quotient form and the 4-dimensional
// ladder: ONE decomposition and ONE plan per wave serve the choice and the ladder
TC_HD_NOINLINE G2Jac combine_divide_cheapest(const G2Jac& a, uint64_t d_abs, bool& exc) {
  d_abs = wave_uniform(d_abs);  // (an argument arrives in vector registers: the decomposition and the plan are scalar work from here)
  uint64_t q = 0;
  int64_t T[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
  bool planned = combine_quotient_decompose(d_abs, &q, T, E);
  QuotPlan plan{0, kQuotWidth, 0};
  if (planned) {
    // (the decomposition divides, which the vector unit does: its results come back to scalar registers for the plan)
    q = wave_uniform(q);
    TC_UNROLL for (int j = 0; j < 4; j++) {
      T[j] = (int64_t)wave_uniform((uint64_t)T[j]);
      E[j] = (int64_t)wave_uniform((uint64_t)E[j]);
    }
    plan = combine_quotient_plan(q, T, E);
    planned = plan.macs < combine_divide_uniform_macs(d_abs);
#if !defined(__HIPCC__)
    if (g_tc_force_divide_form) planned = g_tc_force_divide_form == 2;
#endif
  }
  if (planned) return combine_divide_planned(a, q, T, E, plan, exc);
  return combine_divide_uniform(a, d_abs, exc);
}
TC_HD bool combine_divide_takes_quotient(uint64_t d_abs) {
  uint64_t q;
  int64_t T[4], E[4];
  if (!combine_quotient_decompose(d_abs, &q, T, E)) return false;
#if !defined(__HIPCC__)
  if (g_tc_force_divide_form) return g_tc_force_divide_form == 2;
#endif
  return combine_divide_quotient_macs(q, T, E) < combine_divide_uniform_macs(d_abs);
}

template <class F>
struct IsG2 {
  static constexpr bool V = false;
};
template <>
struct IsG2<Fq2> {
  static constexpr bool V = true;
};
// The combination of a wave whose live jobs all have ONE index tuple (G2; the coefficients c_k and D are then the wave's):
// the table-free short ladder (tc_threshold.h straus_small_uniform) and, for a generic denominator, the cheaper of the two
// [1 / D] forms above (the planned ladder over |x| / D for the small denominators of node numbers, the width-4 NAF ladder
// otherwise: combine_divide_cheapest).
// Lanes that raise an exception flag are recomputed by the forms every other wave runs.
#if !defined(__HIPCC__)
inline int g_tc_force_mixed_combine = 0;  // host test build: 1 = take the forms of a mixed wave (on the host one job is a wave)
#endif
template <int K>
TC_HD G2Jac combine_uniform_wave(const G2Affine* pts, const uint64_t* c_abs, uint64_t d_abs, bool d_neg) {
  bool exc = false;
  G2Jac a = straus_small_uniform<Fq2, K>(pts, c_abs, exc);
  if (wave_any(exc)) a = G2Jac::select(exc, straus_small_call<Fq2, K>(pts, c_abs), a);
  TC_MARK(2);
  const uint64_t du = wave_uniform(d_abs);
  if (combine_denominator_class(du) != kCombineClassGeneric) return combine_divide_call(a, d_abs, d_neg);
  exc = false;
  G2Jac q = combine_divide_cheapest(a, du, exc);
  q.y = Fq2::select(d_neg, -q.y, q.y);
  if (wave_any(exc)) q = G2Jac::select(exc, combine_divide_call(a, d_abs, d_neg), q);
  return q;
}
// every lane that reaches this (the wave's live jobs with decodable shares) holds the same tuple?
template <int K>
TC_HD bool combine_wave_is_uniform(const uint64_t* idx) {
#if !defined(__HIPCC__)
  if (g_tc_force_mixed_combine) return false;
#endif
  uint64_t key = 0;
  TC_UNROLL for (int k = 0; k < K; k++) key |= (idx[k] & 0xffffull) << (16 * k);  // (the fast path took the job: every index < 65 535)
  return !wave_any(key != wave_uniform(key));
}

// Where a job body finds the encodings of its operands and where its result goes.  DirectIO addresses global
// memory as it is (one job per lane: 96/192-byte records `stride` apart); the kernels pass tc_stage.h's WaveRowIO
// instead, which moves whole-wave rows through LDS with coalesced 8-byte loads and stores.  Every lane of a wave
// -- live or not -- must make the same sequence of operand() / result() / commit(wrote) calls.
struct DirectIO {
  const uint8_t* in;
  size_t stride;
  uint8_t* out;
  TC_HD const uint8_t* operand(int k) const { return in + (size_t)k * stride; }
  TC_HD uint8_t* result() const { return out; }
  TC_HD void commit(bool) const {}
};

// combination through the small-index fast path (tc_threshold.h); false => not applicable (or !live)
template <class F, int K, class IO, bool ARENA = false>
TC_HD bool job_combine_small_io(const uint64_t* idx, bool live, IO& io, uint8_t* status) {
  uint64_t c_abs[K], d_abs = 1;
  bool c_neg[K], d_neg = false;
  TC_UNROLL for (int k = 0; k < K; k++) {
    c_abs[k] = 0;
    c_neg[k] = false;
  }
  TC_MARK(0);
  TC_MARK_WALL(8);
  const bool applies = live && lagrange_small_coeffs<K>(idx, c_abs, c_neg, &d_abs, &d_neg);
  Affine<F> pts[K];
  bool ok = true;
  TC_NOUNROLL for (int k = 0; k < K; k++) {
    const uint8_t* enc = io.operand(k);  // wave-uniform: stages share k of every job of the wave
    if (applies) {
      ok &= PointIO<F>::decode(enc, pts[k]);
      if (c_neg[k]) pts[k].y = (-pts[k].y).norm();
    }
  }
  uint8_t* dst = io.result();
  TC_MARK(1);
  if (applies) {
    if (!ok) {
      PointIO<F>::encode(Affine<F>::infinity(), dst);
      *status = TC_JOB_INVALID_ENCODING;
    } else {
      // (G2: out of line -- its own register allocation: the kernel's private segment drops from 8.0 to 5.6 KB at the
      // same speed; the one-lane G1 kernel measured 3 % slower that way)
      if constexpr (IsG2<F>::V) {
        // a wave of one index tuple (the launch groups them so, k_combine.hip) takes the wave-uniform forms
        Jac<F> q;
        if (combine_wave_is_uniform<K>(idx)) {
          q = combine_uniform_wave<K>(pts, c_abs, d_abs, d_neg);
        } else {
          const Jac<F> a = straus_small_call<F, K>(pts, c_abs);
          TC_MARK(2);
          q = combine_divide(a, d_abs, d_neg);
        }
        TC_MARK(4);
        const Affine<F> qa = jac_to_affine(q);
        TC_MARK(5);
        PointIO<F>::encode(qa, dst);
        *status = TC_JOB_OK;
      } else {
        Jac<F> a = (JobLanes<F>::N > 1) ? straus_small_call<F, K>(pts, c_abs) : straus_small<F, K, ARENA>(pts, c_abs);
        TC_MARK(2);
        const Jac<F> q = ARENA ? combine_divide_arena(a, d_abs, d_neg) : combine_divide(a, d_abs, d_neg);
        TC_MARK(4);
        const Affine<F> qa = jac_to_affine(q);
        TC_MARK(5);
        PointIO<F>::encode(qa, dst);
        *status = TC_JOB_OK;
      }
    }
  }
  io.commit(applies);
  TC_MARK(6);
  TC_MARK_WALL(9);
  return applies;
}
template <class F, int K>
TC_HD bool job_combine_small(const uint64_t* idx, const uint8_t* shares, uint8_t* out, uint8_t* status) {
  DirectIO io{shares, (size_t)PointIO<F>::BYTES, out};
  return job_combine_small_io<F, K>(idx, true, io, status);
}

// class of the job's denominator (kCombineClass*); generic when the fast path does not apply
TC_HD int combine_job_class(const uint64_t* idx, int t) {
  uint64_t c_abs[4], d_abs = 0;
  bool c_neg[4], d_neg;
  bool applies = false;
  if (t == 1) applies = lagrange_small_coeffs<2>(idx, c_abs, c_neg, &d_abs, &d_neg);
  if (t == 2) applies = lagrange_small_coeffs<3>(idx, c_abs, c_neg, &d_abs, &d_neg);
  if (t == 3) applies = lagrange_small_coeffs<4>(idx, c_abs, c_neg, &d_abs, &d_neg);
  return applies ? combine_denominator_class(d_abs) : kCombineClassGeneric;
}

// true when job_combine_small will handle the job (so the Lagrange kernel can skip it)
TC_HD bool combine_small_applies(const uint64_t* idx, int t) {
  uint64_t c_abs[4], d_abs;
  bool c_neg[4], d_neg;
  if (t == 1) return lagrange_small_coeffs<2>(idx, c_abs, c_neg, &d_abs, &d_neg);
  if (t == 2) return lagrange_small_coeffs<3>(idx, c_abs, c_neg, &d_abs, &d_neg);
  if (t == 3) return lagrange_small_coeffs<4>(idx, c_abs, c_neg, &d_abs, &d_neg);
  return false;
}

// ---- grouping the G2 fast path's jobs by index tuple (k_combine.hip) ---------------------------------
// A wave whose jobs all combine over ONE signer subset takes the wave-uniform forms above, so from 4096 jobs on the G2
// launch is ordered by the job's first t + 1 indices: a key of 16 bits per index (the fast path only takes indices below
// 65 535; the jobs it leaves share the key "none"), found in a small open-addressing table in the call's workspace.
// Subset mode needs few enough distinct tuples that padding every group to a whole wave stays cheap; otherwise the
// groups are the three denominator classes, as in G1.
constexpr uint32_t kSubsetSlots = 512;      // table entries (a power of two, twice the groups subset mode allows)
constexpr uint32_t kSubsetMaxGroups = 256;
constexpr uint32_t kSubsetPad = 32;         // jobs of a G2 wave
constexpr uint32_t kClassPad = 64;
constexpr uint64_t kTupleKeyNone = ~0ull;
constexpr int kGroupOrders = 4;             // generic, 2^a, 1, none: the expensive waves start first
// the job's key, and the class of its denominator (generic when the fast path does not take it)
TC_HD uint64_t combine_tuple_key(const uint64_t* idx, int t, int* cls) {
  uint64_t c_abs[4], d_abs = 0;
  bool c_neg[4], d_neg;
  bool applies = false;
  if (t == 1) applies = lagrange_small_coeffs<2>(idx, c_abs, c_neg, &d_abs, &d_neg);
  if (t == 2) applies = lagrange_small_coeffs<3>(idx, c_abs, c_neg, &d_abs, &d_neg);
  if (t == 3) applies = lagrange_small_coeffs<4>(idx, c_abs, c_neg, &d_abs, &d_neg);
  *cls = applies ? combine_denominator_class(d_abs) : kCombineClassGeneric;
  if (!applies) return kTupleKeyNone;
  uint64_t key = 0;
  for (int k = 0; k <= t; k++) key |= idx[k] << (16 * k);  // distinct indices: never zero, the table's "empty"
  return key;
}
TC_HD int combine_class_order(int cls) { return cls == kCombineClassGeneric ? 0 : cls == kCombineClassPow2 ? 1 : 2; }
TC_HD int combine_key_order(uint64_t key, int t) {
  if (key == kTupleKeyNone) return 3;
  uint64_t idx[4];
  for (int k = 0; k < 4; k++) idx[k] = (key >> (16 * k)) & 0xffffull;
  return combine_class_order(combine_job_class(idx, t));
}
// ---- what one job of a tuple will execute, predicted (multiply-adds, as profiles/combine_uniform_macs.json counts them) -----
// The launch order of k_combine_plan ranks the groups by it; only the ranking matters.  Built from what the wave itself
// will run: the short ladder of straus_small_uniform (one doubling per column below the top of the longest NAF, one mixed
// addition per nonzero digit but the first), then per class
//   generic   the cheaper of the planned quotient form and the 4-dimensional ladder, exactly as combine_divide_cheapest chooses
//   2^a       psi^3(Q) - psi(Q), the 15 doublings of the positioning loop (all executed, 16 - a of them kept), the 47
//             doublings and 5 additions of |x| >> 16 (combine_divide): as long as a generic chain, whatever a
//   1         nothing
// and the decoding, the one inversion and the encoding every job has (kMacsJobFixed: D = 1 less its short ladder).
constexpr uint32_t kMacsJobFixed = 30002, kMacsPow2Fixed = 25088, kMacsMixedGeneric = 1540687;
template <int K>
TC_HD uint32_t combine_short_ladder_macs(const uint64_t* c_abs) {
  uint64_t any = 0;
  int nz = 0;
  for (int k = 0; k < K; k++) {
    uint64_t pos, neg;
    naf_recode(c_abs[k], &pos, &neg);
    any |= pos | neg;
    nz += __builtin_popcountll(pos | neg);
  }
  const int top = any ? 63 - (int)__builtin_clzll(any) : 0;
  return (uint32_t)top * kMacsDbl + (uint32_t)(nz > 0 ? nz - 1 : 0) * kMacsAdd;
}
TC_HD uint32_t combine_divide_macs(uint64_t d_abs) {
  const int cls = combine_denominator_class(d_abs);
  if (cls == kCombineClassOne) return 0;
  if (cls == kCombineClassPow2) return kMacsPow2Fixed + (15 + 47) * kMacsDbl + 5 * kMacsAdd;
  uint64_t q = 0;
  int64_t T[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
  const bool taken = combine_quotient_decompose(d_abs, &q, T, E);
  const uint32_t planned = taken ? combine_quotient_plan(q, T, E).macs : 0xffffffffu;
  // (the quotient form wins for every D below 2^13 or so -- every denominator of node numbers: no 256-bit inverse and no
  // GLS decomposition for those in the one workgroup of k_combine_plan)
  if (taken && d_abs < (1ull << 12)) return planned;
  const uint32_t ladder = combine_divide_uniform_macs(d_abs);
  return planned < ladder ? planned : ladder;
}
// 0: the fast path does not take the tuple
TC_HD uint32_t combine_tuple_macs(const uint64_t* idx, int t) {
  uint64_t c_abs[4], d_abs = 0;
  bool c_neg[4], d_neg;
  uint32_t ladder = 0;
  bool applies = false;
  if (t == 1 && (applies = lagrange_small_coeffs<2>(idx, c_abs, c_neg, &d_abs, &d_neg))) ladder = combine_short_ladder_macs<2>(c_abs);
  if (t == 2 && (applies = lagrange_small_coeffs<3>(idx, c_abs, c_neg, &d_abs, &d_neg))) ladder = combine_short_ladder_macs<3>(c_abs);
  if (t == 3 && (applies = lagrange_small_coeffs<4>(idx, c_abs, c_neg, &d_abs, &d_neg))) ladder = combine_short_ladder_macs<4>(c_abs);
  if (!applies) return 0;
  return kMacsJobFixed + ladder + combine_divide_macs(d_abs);
}
// the same from a group's key; the group "none" (and an empty entry) counts as a mixed wave of the generic class
TC_HD uint32_t combine_key_macs(uint64_t key, int t) {
  if (key == kTupleKeyNone || key == 0) return kMacsMixedGeneric;
  uint64_t idx[4];
  for (int k = 0; k < 4; k++) idx[k] = (key >> (16 * k)) & 0xffffull;
  const uint32_t m = combine_tuple_macs(idx, t);
  return m ? m : kMacsMixedGeneric;
}
TC_HD uint32_t combine_key_hash(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40); }
TC_HD bool combine_subset_mode(bool overflow, uint32_t groups, size_t B) {
  return !overflow && groups <= kSubsetMaxGroups && (size_t)kSubsetPad * groups <= B / 8;  // padding: at most an eighth of the slots
}
// first slot of group s: the groups sorted by (order, number), each padded to a multiple of `pad` (an empty one takes nothing)
TC_HD uint32_t combine_group_start(const uint32_t* count, const uint8_t* order, uint32_t n, uint32_t s, uint32_t pad) {
  uint32_t start = 0;
  for (uint32_t g = 0; g < n; g++) {
    const bool before = order[g] < order[s] || (order[g] == order[s] && g < s);
    if (before) start += (count[g] + pad - 1) / pad * pad;
  }
  return start;
}

// ---- the pieces of the grouping kernels (k_combine.hip k_combine_group / k_combine_plan) ------------------------------
// Written over arrays so that g++ runs them too (tests/group): on the device the arrays are LDS and the call's workspace and
// the accesses below are atomics; on the host one thread runs the jobs one after the other and they are plain accesses.
#if defined(__HIP_DEVICE_COMPILE__)
TC_HD uint64_t group_cas64(uint64_t* p, uint64_t expect, uint64_t val) {
  return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expect, (unsigned long long)val);
}
TC_HD uint32_t group_add32(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
TC_HD void group_set32(uint32_t* p, uint32_t v) { atomicExch(p, v); }
TC_HD uint32_t group_load32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
TC_HD uint64_t group_load64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
TC_HD uint64_t group_cas64(uint64_t* p, uint64_t expect, uint64_t val) {
  const uint64_t cur = *p;
  if (cur == expect) *p = val;
  return cur;
}
TC_HD uint32_t group_add32(uint32_t* p, uint32_t v) {
  const uint32_t cur = *p;
  *p = cur + v;
  return cur;
}
TC_HD void group_set32(uint32_t* p, uint32_t v) { *p = v; }
TC_HD uint32_t group_load32(const uint32_t* p) { return *p; }
TC_HD uint64_t group_load64(const uint64_t* p) { return *p; }
#endif
// The call's workspace, in words (zeroed by the launcher for every call): the table's keys (64 bits each), the jobs per entry,
// the first slot per entry, then single words.  kGwsNeed: the jobs the fast path leaves (key "none"), for the Lagrange stage
// and the two-stage kernels behind it.
// kGwsStart: subset mode, the group's first WAVE in the launch order; kGwsFold: the resident waves the order folds at, 0 = no fold.
constexpr uint32_t kGwsCount = 2 * kSubsetSlots, kGwsStart = 3 * kSubsetSlots, kGwsMisc = 4 * kSubsetSlots;
constexpr uint32_t kGwsClassCount = kGwsMisc, kGwsClassStart = kGwsMisc + 4, kGwsGroups = kGwsMisc + 8, kGwsOverflow = kGwsMisc + 9,
                   kGwsMode = kGwsMisc + 10, kGwsNeed = kGwsMisc + 11, kGwsFold = kGwsMisc + 12, kGwsZeroWords = kGwsMisc + 16;
// A workgroup takes kGroupWgJobs jobs and first counts them per key in a table of its own (twice as many entries as jobs, so a
// probe always meets the key or an empty entry); then ONE lane per distinct key does the key's work on the call's table.
constexpr uint32_t kGroupWgJobs = 256;
constexpr uint32_t kGroupWgSlots = 2 * kGroupWgJobs;
// (bits of the hash the call's table does not use: keys that meet there are spread here)
TC_HD uint32_t combine_wg_hash(uint64_t key) { return (combine_key_hash(key) >> 9) & (kGroupWgSlots - 1); }
// One job's step (wkey / wcount: kGroupWgSlots zeroed entries): the entry of its key, its rank among the workgroup's jobs of
// that key, and whether this job made the entry -- the job that did is the key's lane in combine_wg_publish.
TC_HD uint32_t combine_wg_insert(uint64_t* wkey, uint32_t* wcount, uint64_t key, uint32_t* local_rank, bool* made) {
  uint32_t s = combine_wg_hash(key);
  *made = false;
  for (uint32_t probe = 0; probe < kGroupWgSlots; probe++) {
    const uint64_t cur = group_cas64(&wkey[s], 0ull, key);
    if (cur == 0) *made = true;
    if (cur == 0 || cur == key) break;
    s = (s + 1) & (kGroupWgSlots - 1);
  }
  *local_rank = group_add32(&wcount[s], 1u);
  return s;
}
// The probe of the call's table starts at the low bits of the hash and advances by an odd step taken from its top bits (every
// entry is visited once in kSubsetSlots steps).  The keys are small indices in 16-bit fields and the low bits of their hashes
// cluster: the 210 four-subsets of ten signers start at 123 entries, and one entry further per step left the last key 41
// steps from home -- every step a dependent round trip to memory, and with every workgroup of a launch inserting into the
// empty table at once a run grows one key per round trip.  With a step of its own per key the longest probe of that batch
// is 6 steps; k_combine_group took 0.084 ms with the one and 0.041 ms with the other (profiles/combine_group_ab.txt).
TC_HD uint32_t combine_probe_step(uint64_t key) { return ((combine_key_hash(key) >> 15) & (kSubsetSlots - 1)) | 1u; }
// The key's entry in the call's table: open addressing, the probing bounded by the table's size.  kSubsetSlots when there is
// none (the table is full, or an earlier key closed it); more than kSubsetMaxGroups keys, or a full table, raise the overflow
// flag -- the plan then orders the jobs by class and no entry is used.
TC_HD uint32_t combine_table_entry(uint32_t* ws, uint64_t key) {
  uint64_t* keys = reinterpret_cast<uint64_t*>(ws);
  if (group_load32(&ws[kGwsOverflow]) != 0) return kSubsetSlots;
  uint32_t h = combine_key_hash(key) & (kSubsetSlots - 1);
  const uint32_t step = combine_probe_step(key);
  for (uint32_t probe = 0; probe < kSubsetSlots; probe++) {
    uint64_t cur = group_load64(&keys[h]);
    if (cur == 0) {
      cur = group_cas64(&keys[h], 0ull, key);
      if (cur == 0) {  // a new group
        cur = key;
        if (group_add32(&ws[kGwsGroups], 1u) >= kSubsetMaxGroups) group_set32(&ws[kGwsOverflow], 1u);
      }
    }
    if (cur == key) return h;
    h = (h + step) & (kSubsetSlots - 1);
  }
  group_set32(&ws[kGwsOverflow], 1u);  // the table is full
  return kSubsetSlots;
}
// The lane that made entry s of the workgroup's table, once every job of the workgroup is counted: the key's entry in the
// call's table and, with ONE addition of the workgroup's count, the rank of the workgroup's first job of the key.
TC_HD void combine_wg_publish(uint32_t s, const uint64_t* wkey, const uint32_t* wcount, uint16_t* wentry, uint32_t* wbase, uint32_t* ws) {
  const uint64_t key = wkey[s];
  if (key == kTupleKeyNone) group_add32(&ws[kGwsNeed], wcount[s]);
  const uint32_t h = combine_table_entry(ws, key);
  wentry[s] = (uint16_t)h;
  wbase[s] = h < kSubsetSlots ? group_add32(&ws[kGwsCount + h], wcount[s]) : 0;
}

// combine_group_start for every group at once, as a prefix sum per order instead of n walks over n counts.  These are the
// steps of n threads with a barrier after each (the host runs step after step, thread after thread); buf: 2 n rows of
// kGroupOrders words.
//   step 0                     row s = the padded size of group s in the column of its order, zero in the others
//   step k = 1 .. L, 2^L >= n  row s of this step = row s + row s - 2^(k-1) of the step before (the two halves of buf alternate)
//   combine_scan_start         the totals of the orders before the group's own + what its own column holds in front of it
TC_HD int combine_scan_steps(uint32_t n) {
  int L = 0;
  while ((1u << L) < n) L++;
  return L + 1;
}
TC_HD void combine_scan_step(int step, uint32_t s, uint32_t n, const uint32_t* count, const uint8_t* order, uint32_t pad, uint32_t* buf) {
  if (step == 0) {
    for (int o = 0; o < kGroupOrders; o++) buf[s * kGroupOrders + o] = (int)order[s] == o ? (count[s] + pad - 1) / pad * pad : 0;
    return;
  }
  const uint32_t d = 1u << (step - 1);
  const uint32_t* src = buf + (size_t)((step - 1) & 1) * n * kGroupOrders;
  uint32_t* dst = buf + (size_t)(step & 1) * n * kGroupOrders;
  for (int o = 0; o < kGroupOrders; o++) dst[s * kGroupOrders + o] = src[s * kGroupOrders + o] + (s >= d ? src[(s - d) * kGroupOrders + o] : 0);
}
TC_HD uint32_t combine_scan_start(uint32_t s, uint32_t n, const uint32_t* count, const uint8_t* order, uint32_t pad, const uint32_t* buf) {
  const uint32_t* sum = buf + (size_t)((combine_scan_steps(n) - 1) & 1) * n * kGroupOrders;  // inclusive sums, where the last step left them
  uint32_t start = sum[s * kGroupOrders + order[s]] - (count[s] + pad - 1) / pad * pad;
  for (int o = 0; o < (int)order[s]; o++) start += sum[(n - 1) * kGroupOrders + o];
  return start;
}

// ---- the launch order of subset mode: by predicted cost, folded once (k_combine_plan / k_combine_place) -------
// The dispatcher hands workgroups out in index order, one per SIMD before any SIMD gets its second, so with `seats` resident
// waves wave k < seats / 2 shares its SIMD with wave k + seats / 2 (tools/placement_probe, profiles/placement_probe.txt), and a
// SIMD that holds waves of lone cost a >= b is busy for a + b / 2.  The order: all waves by descending cost (combine_key_macs);
// and when the launch is ONE resident round with a surplus (combine_order_aligned) the second half of the round is turned
// round, so that the lightest wave of the round sits beside the heaviest -- wave d of the descending sequence goes to slot
//     d                        d < seats / 2 (the heaviest, one per SIMD)  or  d >= seats (the cheapest: they fill what frees first)
//     3 seats / 2 - 1 - d      otherwise
// A group's waves stay one run, or two where the sequence folds; no wave holds two groups; the padding is what it was.
// (The scan above orders by class alone: it stays for the host suites that pin it and for nothing else.)
TC_HD uint32_t combine_group_waves(uint32_t count, uint32_t pad) { return (count + pad - 1) / pad; }
// first wave of group s in the descending sequence (by cost, then by number; empty groups take nothing); *total: all waves
TC_HD uint32_t combine_order_start(const uint32_t* cost, const uint32_t* count, uint32_t n, uint32_t s, uint32_t pad, uint32_t* total) {
  uint32_t start = 0, all = 0;
  for (uint32_t g = 0; g < n; g++) {
    const uint32_t w = combine_group_waves(count[g], pad);
    all += w;
    if (cost[g] > cost[s] || (cost[g] == cost[s] && g < s)) start += w;
  }
  *total = all;
  return start;
}
// one resident round with a surplus of at most 3/16 of it: in the model (tools/sim_launch_order.py, profiles/combine_order_model.txt)
// the fold wins up to 1.18 x seats waves and loses from 1.21 x on, where the surplus no longer fits behind the cheap half; with
// fewer waves than seats there is no pair to choose, and over several rounds plain descending cost is as good
TC_HD bool combine_order_aligned(uint32_t waves, uint32_t seats) { return seats >= 2 && waves >= seats && (uint64_t)16 * waves <= (uint64_t)19 * seats; }
TC_HD uint32_t combine_fold_wave(uint32_t d, uint32_t fold_seats) {
  const uint32_t half = fold_seats / 2;  // (fold_seats = 0: no fold)
  return d >= half && d < 2 * half ? 3 * half - 1 - d : d;
}
// the slot of the job of rank `rank` in a group whose first wave is `start_wave`
TC_HD size_t combine_order_slot(uint32_t start_wave, uint32_t rank, uint32_t pad, uint32_t fold_seats) {
  return (size_t)combine_fold_wave(start_wave + rank / pad, fold_seats) * pad + rank % pad;
}

// out = sum_{i <= t} lambda_i * share_i over the FIRST t+1 samples of the job
// (interpolate, src/lib.rs:719-767).  lam: (t+1) x 8 canonical words from job_lagrange.
// t == 0: the first sample is returned unchanged (src/lib.rs:735-737) -- decoded and encoded again, so a bad encoding fails
template <class F>
TC_HD uint8_t job_first_sample(const uint8_t* shares, uint8_t* out) {
  Affine<F> p;
  if (!PointIO<F>::decode(shares, p)) {
    PointIO<F>::encode(Affine<F>::infinity(), out);
    return TC_JOB_INVALID_ENCODING;
  }
  PointIO<F>::encode(p, out);
  return TC_JOB_OK;
}
// (G1; the G2 general jobs with t >= 1 run through the two-stage kernels of k_msm.hip)
template <class F>
TC_HD uint8_t job_combine(int t, const uint8_t* shares, const uint32_t* lam, uint8_t* out) {
  if (t == 0) return job_first_sample<F>(shares, out);
  return job_lincomb<F>(t + 1, shares, lam, out);
}

// ok = e(a, b) == e(c, d)     (src/lib.rs:109, :185, :511)
TC_HD uint8_t job_pairing_check(const uint8_t* a, const uint8_t* b, const uint8_t* c, const uint8_t* d) {
  G1Affine pa, pc;
  G2Affine qb, qd;
  bool ok = g1_decode_uncompressed(a, pa);
  ok &= g2_decode_uncompressed(b, qb);
  ok &= g1_decode_uncompressed(c, pc);
  ok &= g2_decode_uncompressed(d, qd);
  if (!ok) return 0;
  return pairing_check(pa, qb, pc, qd) ? 1 : 0;
}

// the same with the four operands fetched through IO objects (tc_stage.h: whole-wave rows through LDS); every
// lane of the wave calls the four operand() functions, live or not
template <class IOA, class IOB, class IOC, class IOD>
TC_HD uint8_t job_pairing_check_io(bool live, IOA& a, IOB& b, IOC& c, IOD& d) {
  G1Affine pa = G1Affine::infinity(), pc = G1Affine::infinity();
  G2Affine qb = G2Affine::infinity(), qd = G2Affine::infinity();
  bool ok = live;
  const uint8_t* e = a.operand(0);
  if (live) ok &= g1_decode_uncompressed(e, pa);
  e = b.operand(0);
  if (live) ok &= g2_decode_uncompressed(e, qb);
  e = c.operand(0);
  if (live) ok &= g1_decode_uncompressed(e, pc);
  e = d.operand(0);
  if (live) ok &= g2_decode_uncompressed(e, qd);
  if (!ok) return 0;
  return pairing_check(pa, qb, pc, qd) ? 1 : 0;
}

// The check in two halves (k_pairing.hip runs them as two kernels): the product Miller loop of the two pairs ...
template <class IOA, class IOB, class IOC, class IOD>
TC_HD bool job_miller_io(bool live, IOA& a, IOB& b, IOC& c, IOD& d, Fq12& f) {
  G1Affine pa = G1Affine::infinity(), pc = G1Affine::infinity();
  G2Affine qb = G2Affine::infinity(), qd = G2Affine::infinity();
  bool ok = live;
  const uint8_t* e = a.operand(0);
  if (live) ok &= g1_decode_uncompressed(e, pa);
  e = b.operand(0);
  if (live) ok &= g2_decode_uncompressed(e, qb);
  e = c.operand(0);
  if (live) ok &= g1_decode_uncompressed(e, pc);
  e = d.operand(0);
  if (live) ok &= g2_decode_uncompressed(e, qd);
  if (!ok) {  // the value of an empty product; the caller reports the job as failed
    pa = pc = G1Affine::infinity();
    qb = qd = G2Affine::infinity();
  }
  G1Affine ps[2] = {pa, G1Affine{pc.x, (-pc.y), pc.inf}};
  G2Affine qs[2] = {qb, qd};
  f = miller_loop<2>(ps, qs);
  return ok;
}
// The Miller value of TWO pairs of an n-pair product  prod_k e(a_k, b_k)  (k_pairing.hip k_miller_pairs): no operand is negated
// (NEG: both G1 operands are, for a pair that stands on the other side of the equation); has1 = false: the job's odd last pair,
// whose partner is empty.  Every lane of the wave calls the four operand() functions.  false: an operand did not decode -- the
// value is the empty product and the caller marks the job failed.
template <bool NEG, class IOA, class IOB>
TC_HD bool job_miller_pairs_io(bool has0, bool has1, IOA& a0, IOB& b0, IOA& a1, IOB& b1, Fq12& f) {
  G1Affine ps[2] = {G1Affine::infinity(), G1Affine::infinity()};
  G2Affine qs[2] = {G2Affine::infinity(), G2Affine::infinity()};
  bool ok = true;
  const uint8_t* e = a0.operand(0);
  if (has0) ok &= g1_decode_uncompressed(e, ps[0]);
  e = b0.operand(0);
  if (has0) ok &= g2_decode_uncompressed(e, qs[0]);
  e = a1.operand(0);
  if (has1) ok &= g1_decode_uncompressed(e, ps[1]);
  e = b1.operand(0);
  if (has1) ok &= g2_decode_uncompressed(e, qs[1]);
  if (!ok) {
    ps[0] = ps[1] = G1Affine::infinity();
    qs[0] = qs[1] = G2Affine::infinity();
  }
  if (NEG) {
    ps[0].y = -ps[0].y;
    ps[1].y = -ps[1].y;
  }
  f = miller_loop<2>(ps, qs);
  return ok;
}
// The Miller loop itself in two stages that meet in memory (tc_pairing.h: prepared line products): stage P ...
template <class IOA, class IOB, class IOC, class IOD>
TC_HD bool job_miller_lines_io(bool live, IOA& a, IOB& b, IOC& c, IOD& d, const Fq2Rows& rows) {
  G1Affine pa = G1Affine::infinity(), pc = G1Affine::infinity();
  G2Affine qb = G2Affine::infinity(), qd = G2Affine::infinity();
  bool ok = live;
  const uint8_t* e = a.operand(0);
  if (live) ok &= g1_decode_uncompressed(e, pa);
  e = b.operand(0);
  if (live) ok &= g2_decode_uncompressed(e, qb);
  e = c.operand(0);
  if (live) ok &= g1_decode_uncompressed(e, pc);
  e = d.operand(0);
  if (live) ok &= g2_decode_uncompressed(e, qd);
  if (!ok) {  // the value of an empty product; the caller reports the job as failed
    pa = pc = G1Affine::infinity();
    qb = qd = G2Affine::infinity();
  }
  const G1Affine ps[2] = {pa, G1Affine{pc.x, (-pc.y), pc.inf}};
  const G2Affine qs[2] = {qb, qd};
  const bool skip[2] = {ps[0].inf || qs[0].inf, ps[1].inf || qs[1].inf};
  miller_prepare_lines(ps, qs, skip, rows);
  return ok;
}
// ... stage M: miller_accumulate(rows) ...
// ... and the final exponentiation with the comparison
TC_HD uint8_t job_final_exp_is_one(const Fq12& f) { return final_exponentiation(f) == Fq12::one() ? 1 : 0; }

// hash_g2(msg)      (src/lib.rs:691-694)
// fix = false: the point Q' with hash_g2(msg) = [FR_COFACTOR_FIX] Q' (tc_gls.h g2_clear_cofactor), for the
// composed entry points that fold the constant into a scalar or into the G1 operand of a pairing.
TC_HD G2Jac hash_g2_point(const uint8_t* msg, size_t len, bool fix = true) {
  uint32_t seed[8];
  sha3_256_words(msg, len, seed);
  return g2_random_from_seed(seed, fix);
}
// the same over a per-lane byte buffer (hash_g1_g2): SHA3 out of line (tc_hash.h sha3_256_words_call)
TC_HD G2Jac hash_g2_point_of_buffer(const uint8_t* buf, size_t len, bool fix) {
  uint32_t seed[8];
  sha3_256_words_call(buf, len, seed);
  return g2_random_from_seed(seed, fix);
}
TC_HD void job_hash_g2(const uint8_t* msg, size_t len, uint8_t* out_g2, bool fix = true) {
  g2_encode_uncompressed(jac_to_affine(hash_g2_point(msg, len, fix)), out_g2);
}

// hash_g1_g2(g1, msg)   (src/lib.rs:697-707): the ChaCha20 seed -- sha3_256 of (msg, or its digest beyond 64 bytes) || compress(g1)
TC_HD void hash_g1_g2_seed(const G1Affine& p, const uint8_t* msg, size_t len, uint32_t* seed) {
  uint8_t buf[64 + 48];
  size_t n;
  if (len > 64) {
    uint32_t d[8];
    sha3_256_words_call(msg, len, d);
    for (int i = 0; i < 8; i++) {
      buf[4 * i] = (uint8_t)d[i];
      buf[4 * i + 1] = (uint8_t)(d[i] >> 8);
      buf[4 * i + 2] = (uint8_t)(d[i] >> 16);
      buf[4 * i + 3] = (uint8_t)(d[i] >> 24);
    }
    n = 32;
  } else {
    for (size_t i = 0; i < 64; i++)  // fixed trip count (tc_common.h wave_any)
      if (i < len) buf[i] = msg[i];
    n = len;
  }
  g1_encode_compressed(p, buf + n);
  sha3_256_words_call(buf, n + 48, seed);
}
TC_HD G2Jac hash_g1_g2_point(const G1Affine& p, const uint8_t* msg, size_t len, bool fix = true) {
  uint32_t seed[8];
  hash_g1_g2_seed(p, msg, len, seed);
  return g2_random_from_seed(seed, fix);
}
TC_HD uint8_t job_hash_g1_g2(const uint8_t* g1, const uint8_t* msg, size_t len, uint8_t* out_g2, bool fix = true) {
  G1Affine p;
  if (!g1_decode_uncompressed(g1, p)) {
    // public form: infinity + status.  Internal (fix = false) form, consumed by a pairing check: an
    // encoding that does not decode, so the check fails instead of skipping the pair
    if (fix) g2_encode_uncompressed(G2Affine::infinity(), out_g2);
    else for (int i = 0; i < 192; i++) out_g2[i] = 0xff;
    return TC_JOB_INVALID_ENCODING;
  }
  g2_encode_uncompressed(jac_to_affine(hash_g1_g2_point(p, msg, len, fix)), out_g2);
  return TC_JOB_OK;
}

// ---- two messages per lane pair (tc_duo.h, tc_hash.h g2_random_from_seed_x2): batches from 65 536 messages on ----------------
// SHA3, the streams, the sampling and the Fq exponentiations of message A on lane 0 and of message B on lane 1; out_b may be null
// (an odd batch: the last pair's second slot repeats the first)
TC_HD void hash_g2_x2_finish(const Duo<Seed8>& seed, bool fix, uint8_t* out_a, uint8_t* out_b) {
  G2Jac ra, rb;
  g2_random_from_seed_x2(seed, fix, ra, rb);
  G2Affine pa, pb;
  jac_to_affine_x2(ra, rb, pa, pb);
  g2_encode_uncompressed(pa, out_a);
  if (out_b) g2_encode_uncompressed(pb, out_b);
}
TC_HD void job_hash_g2_x2(const uint8_t* msg_a, size_t len_a, const uint8_t* msg_b, size_t len_b, uint8_t* out_a, uint8_t* out_b,
                          bool fix = true) {
  const Duo<const uint8_t*> msg = duo_pick(msg_a, msg_b);
  const Duo<size_t> len = duo_pick(len_a, len_b);
  Duo<Seed8> seed;
  duo_each([&](int s) { sha3_256_words_call(msg.at(s), len.at(s), seed.at(s).w); });
  hash_g2_x2_finish(seed, fix, out_a, out_b);
}
TC_HD void job_hash_g1_g2_x2(const uint8_t* g1_a, const uint8_t* msg_a, size_t len_a, const uint8_t* g1_b, const uint8_t* msg_b,
                             size_t len_b, uint8_t* out_a, uint8_t* out_b, bool fix, uint8_t& st_a, uint8_t& st_b) {
  const Duo<const uint8_t*> g1 = duo_pick(g1_a, g1_b), msg = duo_pick(msg_a, msg_b);
  const Duo<size_t> len = duo_pick(len_a, len_b);
  Duo<Seed8> seed;
  Duo<bool> decoded;
  duo_each([&](int s) {
    G1Affine p;
    decoded.at(s) = g1_decode_uncompressed(g1.at(s), p);
    if (!decoded.at(s)) p = G1Affine::infinity();  // stand-in: the slot's result is replaced below
    hash_g1_g2_seed(p, msg.at(s), len.at(s), seed.at(s).w);
  });
  hash_g2_x2_finish(seed, fix, out_a, out_b);
  bool oka, okb;
  duo_to(decoded, oka, okb);
  // an undecodable G1 operand: as job_hash_g1_g2 -- infinity + status (public form) / an encoding that does not decode (internal form)
  if (!oka) {
    if (fix) g2_encode_uncompressed(G2Affine::infinity(), out_a);
    else for (int i = 0; i < 192; i++) out_a[i] = 0xff;
  }
  if (!okb && out_b) {
    if (fix) g2_encode_uncompressed(G2Affine::infinity(), out_b);
    else for (int i = 0; i < 192; i++) out_b[i] = 0xff;
  }
  st_a = oka ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  st_b = okb ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// out[i] = data[i] ^ (u8) ChaCha20(sha3_256(compress(g1))).next_u32()   (src/lib.rs:710-715)
TC_HD uint8_t job_xor_with_hash(const uint8_t* g1, const uint8_t* data, size_t len, uint8_t* out) {
  G1Affine p;
  if (!g1_decode_uncompressed(g1, p)) return TC_JOB_INVALID_ENCODING;
  uint8_t comp[48];
  g1_encode_compressed(p, comp);
  uint32_t seed[8];
  sha3_256_words(comp, 48, seed);
  ChaChaRng rng;
  rng.init(seed);
  KeystreamBytes ks;
  size_t i = 0;
  TC_NOUNROLL while (wave_any(i < len)) {
    if (i < len) {
      out[i] = data[i] ^ ks.next(rng);
      i++;
    }
  }
  return TC_JOB_OK;
}

// uncompressed -> compressed (to_bytes, src/lib.rs:149-153, 255-259)
template <class F>
TC_HD uint8_t job_compress(const uint8_t* in, uint8_t* out);
template <>
TC_HD uint8_t job_compress<Fq>(const uint8_t* in, uint8_t* out) {
  G1Affine p;
  bool ok = g1_decode_uncompressed(in, p);
  if (!ok) p = G1Affine::infinity();
  g1_encode_compressed(p, out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
template <>
TC_HD uint8_t job_compress<Fq2>(const uint8_t* in, uint8_t* out) {
  G2Affine p;
  bool ok = g2_decode_uncompressed(in, p);
  if (!ok) p = G2Affine::infinity();
  g2_encode_compressed(p, out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// (u, v, w) = pk.encrypt_with_rng(rng, msg) with the rng's Fr draw r supplied by the caller
// (src/lib.rs:128-137):  u = r g1;  v = msg ^ keystream(r pk);  w = r hash_g1_g2(u, v)
TC_HD uint8_t job_encrypt(const uint8_t* pk96, const uint8_t* r_le32, const uint8_t* msg, size_t len, uint8_t* out_u,
                          uint8_t* out_v, uint8_t* out_w) {
  uint32_t k[8];
  G1Affine pk;
  bool ok = fr_from_le32(r_le32, k);
  ok &= g1_decode_uncompressed(pk96, pk);
  if (!ok) {
    g1_encode_uncompressed(G1Affine::infinity(), out_u);
    g2_encode_uncompressed(G2Affine::infinity(), out_w);
    size_t i = 0;
    TC_NOUNROLL while (wave_any(i < len)) {
      if (i < len) out_v[i++] = 0;
    }
    return TC_JOB_INVALID_ENCODING;
  }
  const G1Affine u = jac_to_affine(g1_mul_glv(g1_generator(), k));
  g1_encode_uncompressed(u, out_u);
  uint8_t g[96];
  g1_encode_uncompressed(jac_to_affine(g1_mul_glv(pk, k)), g);
  job_xor_with_hash(g, msg, len, out_v);
  // (G2 values never round-trip through a per-lane byte buffer: in the lane-pair build each
  // lane only holds half of an encoding)
  // w = [r] [c] Q' = [r c mod r] Q': the cofactor-fix multiplication of the hash folds into this one
  uint32_t kc[8];
  fr_mul_cofactor_fix(k, kc);
  g2_encode_uncompressed(jac_to_affine(g2_mul_gls(hash_g1_g2_point(u, out_v, len, false), kc)), out_w);
  return TC_JOB_OK;
}

// Commitment::evaluate(i + 1) (src/poly.rs:497-508) = PublicKeySet::public_key_share(i)
// (src/lib.rs:570-573): Horner in G1, result = result * x + c_k from the top coefficient down,
// x = idx + 1 as a 64-bit ladder (x = 2^64 is handled by the general scalar path of the caller).
TC_HD uint8_t job_commitment_evaluate(const uint8_t* commit, int t, uint64_t idx, uint8_t* out96) {
  const uint64_t x = idx + 1;
  G1Affine c;
  if (x == 0 || !g1_decode_uncompressed(commit + (size_t)t * 96, c)) {
    g1_encode_uncompressed(G1Affine::infinity(), out96);
    return TC_JOB_INVALID_ENCODING;
  }
  G1Jac res = G1Jac::from_affine(c);
  bool ok = true;
  TC_NOUNROLL for (int kk = t - 1; kk >= 0; kk--) {
    // res = res * x
    G1Jac acc = G1Jac::infinity();
    bool started = false;
    TC_NOUNROLL for (int bit = 63; bit >= 0; bit--) {
      if (started) acc = jac_dbl(acc);
      if ((x >> bit) & 1ull) {
        acc = started ? jac_add(acc, res) : res;
        started = true;
      }
    }
    ok &= g1_decode_uncompressed(commit + (size_t)kk * 96, c);
    res = jac_add_mixed(acc, c);
  }
  if (!ok) {
    g1_encode_uncompressed(G1Affine::infinity(), out96);
    return TC_JOB_INVALID_ENCODING;
  }
  g1_encode_uncompressed(jac_to_affine(res), out96);
  return TC_JOB_OK;
}

// compressed -> uncompressed with the reference's CHECKED decode (from_bytes,
// src/lib.rs:140-146, 246-252): on the curve and in the order-r subgroup, else Invalid
template <class F>
TC_HD uint8_t job_decompress(const uint8_t* in, uint8_t* out);
template <>
TC_HD uint8_t job_decompress<Fq>(const uint8_t* in, uint8_t* out) {
  G1Affine p;
  bool ok = g1_decode_compressed(in, p);
  if (!ok) p = G1Affine::infinity();
  g1_encode_uncompressed(p, out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
template <>
TC_HD uint8_t job_decompress<Fq2>(const uint8_t* in, uint8_t* out) {
  G2Affine p;
  bool ok = g2_decode_compressed(in, p);
  if (!ok) p = G2Affine::infinity();
  g2_encode_uncompressed(p, out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// the same for TWO compressed G2 points on one lane pair (tc_duo.h: the Fq exponentiations of the two square roots run on one
// lane each); out_b may be null (an odd point count: the pair's second slot repeats the first)
TC_HD void job_decompress_g2_x2(const uint8_t* in_a, const uint8_t* in_b, uint8_t* out_a, uint8_t* out_b, uint8_t& st_a, uint8_t& st_b) {
  G2Affine pa, pb;
  bool oka, okb;
  g2_decode_compressed_x2(in_a, in_b, pa, pb, oka, okb);
  g2_encode_uncompressed(pa, out_a);
  if (out_b) g2_encode_uncompressed(pb, out_b);
  st_a = oka ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  st_b = okb ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// ---- the selected decode of the wire-level robust combiners (k_mul.hip k_decompress_selected) -------------------------------
// compressed -> uncompressed through the CURVE-LEVEL decode (tc_sqrt.h, MEMBER = false): flags, range, square root and sign,
// no subgroup ladder.  A failure writes the identity.
template <class F>
TC_HD uint8_t job_decompress_curve(const uint8_t* in, uint8_t* out);
template <>
TC_HD uint8_t job_decompress_curve<Fq>(const uint8_t* in, uint8_t* out) {
  G1Affine p;
  bool ok = g1_decode_compressed<false>(in, p);
  if (!ok) p = G1Affine::infinity();
  g1_encode_uncompressed(p, out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
template <>
TC_HD uint8_t job_decompress_curve<Fq2>(const uint8_t* in, uint8_t* out) {
  G2Affine p;
  bool ok = g2_decode_compressed<false>(in, p);
  if (!ok) p = G2Affine::infinity();
  g2_encode_uncompressed(p, out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
// Record i of the selected decode: the share at selected_source (tc_robust.h) of `in`, to out (this record's bytes).  A record
// without a source -- its job lacks enough shares -- reads nothing and is the identity with ok = 1, what k_gather_selected
// gives such a job.  Returns ok.
template <class F>
TC_HD bool job_decompress_selected(const uint8_t* in, size_t N, size_t need, const uint32_t* slot, const uint8_t* enough, size_t i, uint8_t* out) {
  const size_t src = selected_source(i, N, need, slot, enough, PointIO<F>::CBYTES);
  if (src == kNoSource) {
    PointIO<F>::encode(Affine<F>::infinity(), out);
    return true;
  }
  return job_decompress_curve<F>(in + src, out) == TC_JOB_OK;
}
// Records ia and ib (ib == ia: an odd record count, the second slot repeats the first and out_b is null) on one lane pair.  The
// two may belong to different jobs; a record without a source borrows the other's bytes for the shared arithmetic and is
// replaced by the identity before anything is written; two without a source decode nothing.
TC_HD void job_decompress_selected_g2_x2(const uint8_t* in, size_t N, size_t need, const uint32_t* slot, const uint8_t* enough, size_t ia, size_t ib,
                                         uint8_t* out_a, uint8_t* out_b, bool& oka, bool& okb) {
  const size_t sa = selected_source(ia, N, need, slot, enough, 96), sb = selected_source(ib, N, need, slot, enough, 96);
  G2Affine pa = G2Affine::infinity(), pb = G2Affine::infinity();
  oka = okb = true;
  if (sa != kNoSource || sb != kNoSource) {
    g2_decode_compressed_x2<false>(in + (sa != kNoSource ? sa : sb), in + (sb != kNoSource ? sb : sa), pa, pb, oka, okb);
    if (sa == kNoSource) {
      pa = G2Affine::infinity();
      oka = true;
    }
    if (sb == kNoSource) {
      pb = G2Affine::infinity();
      okb = true;
    }
  }
  g2_encode_uncompressed(pa, out_a);
  if (out_b) g2_encode_uncompressed(pb, out_b);
}

}  // namespace tc
