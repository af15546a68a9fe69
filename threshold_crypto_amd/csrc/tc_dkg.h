// DKG algebra (device side): fixed-base G1 multiplication for Poly::commitment / BivarPoly::commitment
// (/root/reference/src/poly.rs:372-377, 625-632), Horner evaluation of commitment rows for
// BivarCommitment::row / evaluate (:694-727) and the Fr-only Poly::interpolate (:341-350, 388-417).
//
// Poly::commitment multiplies ONE point -- the G1 generator -- by every coefficient, so the window table is
// the same for every job of every batch: it is built once per context and staged in LDS by each workgroup
// (k_dkg.hip).  With signed 4-bit windows
//     k = sum_{w < 64} d_w 16^w,   d_w in [-8, 8],        T[w][m - 1] = [m 16^w] g1   (m = 1 .. 8)
// a multiplication is 64 mixed additions and NO doubling (the reference's CurveAffine::mul: 255 doublings +
// ~127 additions; the variable-base GLV ladder of tc_gls.h: 128 + ~96).  512 affine entries x 112 B = 56 KB
// of LDS, i.e. two 256-lane workgroups per CU.
#pragma once
#include "tc_jobs.h"

namespace tc {

constexpr int kFbWindows = 64;                                      // 4-bit windows of a 256-bit scalar
constexpr int kFbEntries = 8;                                       // |digit| = 1 .. 8
constexpr int kFbPointWords = 2 * FQ_LIMBS;                         // x, y: 28 x int32
constexpr int kFbTableWords = kFbWindows * kFbEntries * kFbPointWords;  // 14 336 words = 57 344 B

// entry e = 8 w + (m - 1) of the table: [m 16^w] g1, affine, limbs carry-normalised
TC_HD void fixed_base_table_entry(int e, int32_t* out28) {
  const int w = e / kFbEntries, m = e % kFbEntries + 1;
  uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int bit = 4 * w;
  k[bit >> 5] = (uint32_t)m << (bit & 31);  // m <= 8 and 4 | bit: never straddles a word
  if (!limbs_lt_p<FrParams>(k)) {  // 8 16^63 = 2^255 > r, and the ladder takes scalars below r: the entry no scalar below r reaches
    uint32_t borrow = 0;
    TC_UNROLL for (int i = 0; i < 8; i++) {
      const uint64_t t = (uint64_t)k[i] - FR_P[i] - borrow;
      borrow = (uint32_t)(t >> 63);
      k[i] = (uint32_t)t;
    }
  }
  const G1Affine p = jac_to_affine(g1_mul_glv(g1_generator(), k));
  const Fq x = p.x.norm(), y = p.y.norm();
  TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) {
    out28[i] = x.l[i];
    out28[FQ_LIMBS + i] = y.l[i];
  }
}

// [k] g1 from the window table (tbl: kFbTableWords int32 in LDS or global memory), k < r as 8 LE words
template <class TBL>
TC_HD G1Jac g1_fixed_base_mul(TBL tbl, const uint32_t* k) {
  G1Jac acc = G1Jac::infinity();
  uint32_t carry = 0;
  TC_NOUNROLL for (int w = 0; w < kFbWindows; w++) {
    const uint32_t v = ((k[w >> 3] >> (4 * (w & 7))) & 15u) + carry;  // 0 .. 16
    const bool neg = v > 8;
    carry = neg ? 1u : 0u;
    const uint32_t mag = neg ? 16u - v : v;  // 0 .. 8
    // k < r < 2^255: the top nibble is at most 7, so the last window absorbs its carry (mag <= 8)
    G1Affine e;
    e.inf = mag == 0;
    const int base = (w * kFbEntries + (int)(mag ? mag - 1 : 0)) * kFbPointWords;
    TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) {
      e.x.l[i] = tbl[base + i];
      e.y.l[i] = tbl[base + FQ_LIMBS + i];
    }
    e.x.set_range(0.f, 1.001f);
    e.x.set_val(2.1f);
    e.y.set_range(0.f, 1.001f);
    e.y.set_val(2.1f);
    e.y = Fq::select(neg, (-e.y).norm(), e.y);
    acc = jac_add_mixed(acc, e);
  }
  return acc;
}

// out = fr * g1   (Poly::commitment src/poly.rs:372-377: `G1Affine::one().mul(*c)`)
template <class TBL>
TC_HD uint8_t job_g1_fixed_base_mul(TBL tbl, const uint8_t* fr_le32, uint8_t* out96) {
  uint32_t k[8];
  if (!fr_from_le32(fr_le32, k)) {
    g1_encode_uncompressed(G1Affine::infinity(), out96);
    return TC_JOB_INVALID_ENCODING;
  }
  g1_encode_uncompressed(jac_to_affine(g1_fixed_base_mul(tbl, k)), out96);
  return TC_JOB_OK;
}

// position of coefficient (i, j) of a symmetric bivariate polynomial (coeff_pos, src/poly.rs:746-750)
TC_HD size_t bivar_coeff_pos(size_t i, size_t j) {
  const size_t lo = i < j ? i : j, hi = i < j ? j : i;
  return lo + hi * (hi + 1) / 2;
}

// res <- res * x  for a 64-bit x (the Horner step of Commitment::evaluate / BivarCommitment::row)
TC_HD G1Jac g1_mul_u64(const G1Jac& p, uint64_t x) {
  G1Jac acc = G1Jac::infinity();
  bool started = false;
  TC_NOUNROLL for (int bit = 63; bit >= 0; bit--) {
    if (started) acc = jac_dbl(acc);
    if ((x >> bit) & 1ull) {
      acc = started ? jac_add(acc, p) : p;
      started = true;
    }
  }
  return acc;
}

// BivarCommitment::row(x)[i] = sum_j commit[pos(i, j)] x^j   (src/poly.rs:713-727), x = IntoFr for u64 (the
// value itself, src/into_fr.rs:16-20), evaluated by Horner from the top coefficient down.
TC_HD uint8_t job_bivar_commitment_row(const uint8_t* commit, size_t degree, size_t i, uint64_t x, uint8_t* out96) {
  G1Affine c;
  bool ok = g1_decode_uncompressed(commit + bivar_coeff_pos(i, degree) * 96, c);
  G1Jac res = G1Jac::from_affine(c);
  TC_NOUNROLL for (size_t jj = degree; jj-- > 0;) {
    G1Jac scaled = g1_mul_u64(res, x);
    ok &= g1_decode_uncompressed(commit + bivar_coeff_pos(i, jj) * 96, c);
    res = jac_add_mixed(scaled, c);
  }
  if (!ok) {
    g1_encode_uncompressed(G1Affine::infinity(), out96);
    return TC_JOB_INVALID_ENCODING;
  }
  g1_encode_uncompressed(jac_to_affine(res), out96);
  return TC_JOB_OK;
}

// ---- Poly::interpolate in Fr (src/poly.rs:388-417 compute_interpolation), one lane per polynomial ------------
// xs, ys: n x 8 canonical LE words; out: n coefficients (low degree first, canonical words; the reference's
// Poly drops trailing zeros, the caller strips them); ws: 2 (n + 1) x 8 words of scratch.  The sample-by-sample
// construction of the reference: `poly` is right on the samples seen so far, `base` vanishes on them.
TC_HD Fr fr_horner(const uint32_t* coeffs_mont, size_t len, const Fr& x) {
  Fr r = Fr::zero();
  TC_NOUNROLL for (size_t k = len; k-- > 0;) {
    Fr c;
    TC_UNROLL for (int i = 0; i < 8; i++) c.v.l[i] = coeffs_mont[k * 8 + i];
    r = r * x + c;
  }
  return r;
}
TC_HD uint8_t job_fr_interpolate(size_t n, const uint32_t* xs, const uint32_t* ys, uint32_t* out, uint32_t* ws) {
  uint32_t* poly = ws;                 // Montgomery form while we work
  uint32_t* base = ws + (n + 1) * 8;
  bool ok = true;
  TC_NOUNROLL for (size_t s = 0; s < n; s++) ok &= limbs_lt_p<FrParams>(xs + s * 8) && limbs_lt_p<FrParams>(ys + s * 8);
  if (!ok || n == 0) {
    TC_NOUNROLL for (size_t k = 0; k < n * 8; k++) out[k] = 0;
    return n == 0 ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  }
  auto put = [](uint32_t* dst, const Fr& v) { TC_UNROLL for (int i = 0; i < 8; i++) dst[i] = v.v.l[i]; };
  auto get = [](const uint32_t* src) { Fr v; TC_UNROLL for (int i = 0; i < 8; i++) v.v.l[i] = src[i]; return v; };
  const Fr x0 = Fr::from_canonical(xs);
  put(poly, Fr::from_canonical(ys));
  put(base, Fr::zero() - x0);
  put(base + 8, Fr::one());
  size_t len_poly = 1, len_base = 2;
  bool dup = false;
  TC_NOUNROLL for (size_t s = 1; s < n; s++) {
    const Fr x = Fr::from_canonical(xs + s * 8), y = Fr::from_canonical(ys + s * 8);
    const Fr bv = fr_horner(base, len_base, x);
    dup = dup || bv.is_zero();  // "sample points must be distinct" (src/poly.rs:404)
    const Fr diff = (y - fr_horner(poly, len_poly, x)) * bv.inv();
    // base *= diff; poly += base
    TC_NOUNROLL for (size_t k = 0; k < len_base; k++) {
      const Fr b = get(base + k * 8) * diff;
      put(base + k * 8, b);
      put(poly + k * 8, (k < len_poly ? get(poly + k * 8) : Fr::zero()) + b);
    }
    len_poly = len_base;
    // base *= (X - x), from the top coefficient down
    put(base + len_base * 8, get(base + (len_base - 1) * 8));
    TC_NOUNROLL for (size_t k = len_base - 1; k > 0; k--) put(base + k * 8, get(base + (k - 1) * 8) - x * get(base + k * 8));
    put(base, Fr::zero() - x * get(base));
    len_base++;
  }
  TC_NOUNROLL for (size_t k = 0; k < n; k++) {
    if (dup) {
      TC_UNROLL for (int i = 0; i < 8; i++) out[k * 8 + i] = 0;
    } else {
      get(poly + k * 8).to_canonical(out + k * 8);
    }
  }
  return dup ? TC_JOB_DUPLICATE_ENTRY : TC_JOB_OK;
}

// ---- DKG verification: the secret side in Fr ------------------------------------------------------------------
// Poly::evaluate (src/poly.rs:358-369) and BivarPoly::row (:607-622), one output scalar per call; the coefficients have
// been brought to Montgomery form once (fr_mont_from_le32), with one validity byte each.
// 32 B LE -> Montgomery words; a non-canonical value (>= r) gives zero and false
TC_HD bool fr_mont_from_le32(const uint8_t* le32, uint32_t* mont8) {
  uint32_t k[8];
  const bool ok = fr_from_le32(le32, k);
  const Fr v = ok ? Fr::from_canonical(k) : Fr::zero();
  TC_UNROLL for (int i = 0; i < 8; i++) mont8[i] = v.v.l[i];
  return ok;
}
TC_HD void fr_store_le32(const Fr& v, uint8_t* out32) {
  uint32_t w[8];
  v.to_canonical(w);
  TC_UNROLL for (int i = 0; i < 8; i++) {
    out32[4 * i] = (uint8_t)w[i];
    out32[4 * i + 1] = (uint8_t)(w[i] >> 8);
    out32[4 * i + 2] = (uint8_t)(w[i] >> 16);
    out32[4 * i + 3] = (uint8_t)(w[i] >> 24);
  }
}
// out = sum_k coeff[k] x^k (n = 0: the zero polynomial); fails -- zero output -- on a non-canonical coefficient or abscissa
TC_HD uint8_t job_fr_poly_evaluate(const uint32_t* coeff_mont, const uint8_t* coeff_valid, size_t n, const uint8_t* x_le32, uint8_t* out32) {
  uint32_t xw[8];
  bool ok = fr_from_le32(x_le32, xw);
  TC_NOUNROLL for (size_t k = 0; k < n; k++) ok &= coeff_valid[k] != 0;
  const Fr r = ok ? fr_horner(coeff_mont, n, Fr::from_canonical(xw)) : Fr::zero();
  fr_store_le32(r, out32);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
// out = row(x)[i] = sum_j coeff[pos(i, j)] x^j over the (degree+1)^2 matrix sq[i][j] = coeff[pos(i, j)] (Montgomery form)
TC_HD uint8_t job_bivar_poly_row(const uint32_t* sq_mont, const uint8_t* sq_valid, size_t degree, size_t i, uint64_t x, uint8_t* out32) {
  const size_t n = degree + 1;
  bool ok = true;
  TC_NOUNROLL for (size_t j = 0; j < n; j++) ok &= sq_valid[i * n + j] != 0;
  const Fr r = ok ? fr_horner(sq_mont + i * n * 8, n, fr_from_u64(x)) : Fr::zero();
  fr_store_le32(r, out32);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// Commitment::evaluate(x) (src/poly.rs:497-508) at the u64 abscissa x BY VALUE -- 0 and 2^64 - 1 included; the idx + 1
// form is job_commitment_evaluate (tc_jobs.h) -- Horner in G1 from the top coefficient down
TC_HD uint8_t job_commitment_evaluate_at(const uint8_t* commit, size_t degree, uint64_t x, uint8_t* out96) {
  G1Affine c;
  bool ok = g1_decode_uncompressed(commit + degree * 96, c);
  G1Jac res = G1Jac::from_affine(c);
  TC_NOUNROLL for (size_t kk = degree; kk-- > 0;) {
    G1Jac scaled = g1_mul_u64(res, x);
    ok &= g1_decode_uncompressed(commit + kk * 96, c);
    res = jac_add_mixed(scaled, c);
  }
  if (!ok) {
    g1_encode_uncompressed(G1Affine::infinity(), out96);
    return TC_JOB_INVALID_ENCODING;
  }
  g1_encode_uncompressed(jac_to_affine(res), out96);
  return TC_JOB_OK;
}

// ---- the combined values check (tc_dkg_verify_values_rlc_batch) -------------------------------------------------
// The n checks  R.evaluate(x_k) == v_k g1  of one part (R: its row commitment, degree+1 points) hold iff, up to 2^-63,
//     sum_i c_i R_i + c_g g1 == 0,     c_i = sum_k rho_k x_k^i  (0^0 = 1),     c_g = - sum_k rho_k v_k
// for secret rho_k: the sum is sum_k rho_k (R.evaluate(x_k) - v_k g1), and a non-zero combination of elements of a group of
// prime order r with coefficients drawn from 2^63 values that are pairwise distinct mod r vanishes with probability <= 2^-63.
// rho_{j,k}: the first two words of ChaCha20(key, block counter j n + k) with the low bit set
TC_HD uint64_t dkg_rlc_rho(const uint32_t* key8, uint64_t counter) {
  ChaChaRng rng;
  rng.init(key8);
  rng.counter = counter;
  const uint32_t w0 = rng.next_u32(), w1 = rng.next_u32();
  return ((uint64_t)w1 << 32) | (uint64_t)(w0 | 1u);
}
// scalar i of job j as 8 canonical words: c_i for i <= degree, c_g for i = degree + 1 (false, and zero -- every one of the
// degree + 2 scalars -- when one of the values is not canonical).  xs, vals: the job's own n abscissae and n x 32 B LE values
TC_HD bool dkg_rlc_scalar(const uint32_t* key8, size_t j, size_t n, size_t degree, const uint64_t* xs, const uint8_t* vals, size_t i,
                          uint32_t* out8) {
  Fr acc = Fr::zero();
  bool ok = true;
  int top = 0;  // the highest set bit of the exponent
  TC_NOUNROLL for (int bit = 1; bit < 64; bit++)
    if ((i >> bit) & 1) top = bit;
  TC_NOUNROLL for (size_t k = 0; k < n; k++) {
    const Fr rho = fr_from_u64(dkg_rlc_rho(key8, (uint64_t)j * n + k));
    Fr term;
    uint32_t v[8];
    ok &= fr_from_le32(vals + k * 32, v);  // every scalar of the job looks at the values: all of them are zero when one is not canonical
    if (i > degree) {
      term = Fr::from_canonical(v);
    } else {
      // x_k^i, left-to-right square and multiply (i = 0: one)
      const Fr x = fr_from_u64(xs[k]);
      term = Fr::one();
      TC_NOUNROLL for (int bit = top; bit >= 0; bit--) {
        term = term.sqr();
        if ((i >> bit) & 1) term = term * x;
      }
    }
    acc = acc + rho * term;
  }
  if (i > degree) acc = Fr::zero() - acc;
  if (!ok) acc = Fr::zero();
  acc.to_canonical(out8);
  return ok;
}
// the degree + 2 scalars of job j (out: (degree+2) x 8 words); false when a value is not canonical
TC_HD bool job_dkg_rlc_scalars(const uint32_t* key8, size_t j, size_t n, size_t degree, const uint64_t* xs, const uint8_t* vals, uint32_t* out) {
  bool ok = true;
  TC_NOUNROLL for (size_t i = 0; i <= degree + 1; i++) ok &= dkg_rlc_scalar(key8, j, n, degree, xs, vals, i, out + i * 8);
  return ok;
}

// ---- DKG finalisation: the accepted parts summed into the key set (src/poly.rs:870-876, 895-898) -----------------------
// Commitment::add_assign (src/poly.rs:462-471) folded over n terms is, per coefficient, a sum of n points: few outputs and long
// sums at the large shape (68 x 200), so an output is split over `parts` adjacent lanes (k_dkg.hip k_g1_sum), lane g summing
// the terms [g n / parts, (g + 1) n / parts) -- msm_part's split (tc_msm.h): every k < n in exactly one lane, a lane with
// parts > n may own nothing.
struct SumPart {
  size_t k0, k1;
};
TC_HD SumPart sum_part(size_t n, size_t g, size_t parts) { return SumPart{g * n / parts, (g + 1) * n / parts}; }

// one lane's partial sum  sum_{k in part, included} pts[k * term_stride]  (pts: the address of term 0 of THIS output).  Term k
// is included when mask is null or mask[k] != 0; an excluded term is not decoded and touches nothing, whatever its bytes.
// member (checked-input mode, else null): member[k * member_stride] == 0 marks a term outside the order-r subgroup.  ok =
// every included term decoded (and was a member); a bad one counts as the identity and, with term_bad, sets term_bad[k] = 1.
// The additions are the complete ones: equal and opposite terms are ordinary inputs (one dealer's commitment twice, P and -P).
TC_HD G1Jac job_g1_sum_part(const uint8_t* pts, size_t term_stride, const uint8_t* mask, const uint8_t* member, size_t member_stride,
                            SumPart part, bool& ok, uint8_t* term_bad = nullptr) {
  G1Jac acc = G1Jac::infinity();
  ok = true;
  TC_NOUNROLL for (size_t k = part.k0; k < part.k1; k++) {
    if (mask && mask[k] == 0) continue;
    G1Affine c;
    bool good = g1_decode_uncompressed(pts + k * term_stride, c);
    if (member) good = good && member[k * member_stride] != 0;
    if (!good) {
      c = G1Affine::infinity();
      if (term_bad) term_bad[k] = 1;
    }
    ok = ok && good;
    acc = jac_add_mixed(acc, c);
  }
  return acc;
}

// out = sum_{k < n, included} vals[k * term_stride] mod r  (Poly::add_assign src/poly.rs:68-80 per coefficient; :876).  The
// terms are canonical residues and addition does not care about the Montgomery factor: no conversion either way.  A
// non-canonical included value: zero output, TC_JOB_INVALID_ENCODING.
TC_HD uint8_t job_fr_sum(const uint8_t* vals, size_t term_stride, size_t n, const uint8_t* mask, uint8_t* out32) {
  Fr acc = Fr::zero();
  bool ok = true;
  TC_NOUNROLL for (size_t k = 0; k < n; k++) {
    if (mask && mask[k] == 0) continue;
    Fr t;
    const bool good = fr_from_le32(vals + k * term_stride, t.v.l);
    if (!good) t = Fr::zero();
    ok = ok && good;
    acc = acc + t;
  }
  if (!ok) acc = Fr::zero();
  TC_UNROLL for (int i = 0; i < 8; i++) {
    out32[4 * i] = (uint8_t)acc.v.l[i];
    out32[4 * i + 1] = (uint8_t)(acc.v.l[i] >> 8);
    out32[4 * i + 2] = (uint8_t)(acc.v.l[i] >> 16);
    out32[4 * i + 3] = (uint8_t)(acc.v.l[i] >> 24);
  }
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// coefficient 0 of job_fr_interpolate's polynomial through the n samples (xs[k] by value, vals[k]): `my_row.evaluate(0)`
// (src/poly.rs:870-876) without the row.  The Lagrange sum  sum_i y_i prod_{j != i} x_j / (x_j - x_i)  kept as ONE fraction
// num / den (num/den + a/b = (num b + a den) / (den b)): no scratch, one inversion.  Statuses as job_fr_interpolate: a
// non-canonical value INVALID_ENCODING, a repeated abscissa (some x_j - x_i = 0, so den = 0) DUPLICATE_ENTRY, n = 0 zero.
TC_HD uint8_t job_fr_interpolate_at_zero(size_t n, const uint64_t* xs, const uint8_t* vals, uint8_t* out32) {
  Fr num = Fr::zero(), den = Fr::one();
  bool ok = true;
  TC_NOUNROLL for (size_t i = 0; i < n; i++) {
    uint32_t w[8];
    const bool good = fr_from_le32(vals + i * 32, w);
    ok = ok && good;
    Fr a = good ? Fr::from_canonical(w) : Fr::zero();
    Fr b = Fr::one();
    const Fr xi = fr_from_u64(xs[i]);
    TC_NOUNROLL for (size_t j = 0; j < n; j++) {
      if (j == i) continue;
      const Fr xj = fr_from_u64(xs[j]);
      a = a * xj;
      b = b * (xj - xi);
    }
    num = num * b + a * den;
    den = den * b;
  }
  const bool dup = den.is_zero();
  const Fr r = (ok && !dup) ? num * den.inv() : Fr::zero();
  fr_store_le32(r, out32);
  return !ok ? TC_JOB_INVALID_ENCODING : dup ? TC_JOB_DUPLICATE_ENTRY : TC_JOB_OK;
}

// ---- DKG resharing: the accepted parts summed with Lagrange weights (`Poly * Fr` src/poly.rs:210-254, Commitment::add_assign
// :462-471, the tail of distributed_key_generation :870-876, 895-898, the coefficients of src/lib.rs:719-767) ---------------------
// A weight is shared by every output of a sum, so it is validated and recoded ONCE per term (k_dkg.hip k_wsum_recode) into
// kWsumWeightWords words: neg (4), u (4) of glv_recode_sign_aligned and the flags below.
constexpr int kWsumWeightWords = 9;
constexpr uint32_t kWsumTop = 1u, kWsumFlip = 2u, kWsumZero = 4u, kWsumValid = 8u;
TC_HD void wsum_recode_weight(const uint8_t* w_le32, uint32_t* rec) {
  uint32_t k[8];
  const bool ok = fr_from_le32(w_le32, k);
  bool zero = true;
  TC_UNROLL for (int i = 0; i < 8; i++) zero = zero && k[i] == 0;
  tc_u128 neg = 0, u = 0;
  bool top = false, flip = false;
  if (ok && !zero) flip = glv_recode_sign_aligned(k, &neg, &u, &top);
  TC_UNROLL for (int i = 0; i < 4; i++) {
    rec[i] = (uint32_t)(neg >> (32 * i));
    rec[4 + i] = (uint32_t)(u >> (32 * i));
  }
  rec[8] = (top ? kWsumTop : 0u) | (flip ? kWsumFlip : 0u) | (zero ? kWsumZero : 0u) | (ok ? kWsumValid : 0u);
}

// the weighted twin of job_g1_sum_part: one lane's partial sum  sum_{k in part, included} w_k pts[k * term_stride], weights as
// wsum_recode_weight left them (rec: term 0's).  Mask, member and term_bad as there: an excluded term is neither decoded nor
// multiplied, and its weight is not looked at.  An included term with a non-canonical weight clears ok -- in the lane that owns
// the term of EVERY output, so every output fails.  Each product is the GLV ladder of tc_g1_mul_batch's routine (g1_mul_glv,
// here from the recoded scalar); a zero weight or an identity term contributes nothing and runs no ladder.  The products are
// folded with the COMPLETE addition: the weights are public, so a dealer can choose its commitment such that w_a P_a = +-w_b P_b.
// A long sum is cut into `slices` consecutive ranges of positions, each with its own group of `parts` lanes (k_g1_wsum): lane g of
// slice s owns sum_part of the slice's range -- every position in exactly one (slice, lane).
TC_HD SumPart wsum_slice_part(size_t n, size_t s, size_t slices, size_t g, size_t parts) {
  const SumPart sl = sum_part(n, s, slices);
  const SumPart in = sum_part(sl.k1 - sl.k0, g, parts);
  return SumPart{sl.k0 + in.k0, sl.k0 + in.k1};
}
// sel (may be null): the sum runs over the terms sel[0 .. n) instead of 0 .. n -- part is then a range of POSITIONS in sel, and
// pts, rec, mask, member and term_bad are still addressed by term (tc_dkg_reshare_batch: the t_old + 1 dealers of S out of P
// parts, spread evenly over the lanes of an output wherever they sit among the parts).
TC_HD G1Jac job_g1_wsum_part(const uint8_t* pts, size_t term_stride, const uint32_t* rec, const uint8_t* mask, const uint8_t* member,
                             size_t member_stride, SumPart part, bool& ok, uint8_t* term_bad = nullptr, const uint32_t* sel = nullptr) {
  G1Jac acc = G1Jac::infinity();
  ok = true;
  TC_NOUNROLL for (size_t pos = part.k0; pos < part.k1; pos++) {
    const size_t k = sel ? (size_t)sel[pos] : pos;
    if (mask && mask[k] == 0) continue;
    G1Affine c;
    bool good = g1_decode_uncompressed(pts + k * term_stride, c);
    if (member) good = good && member[k * member_stride] != 0;
    if (!good && term_bad) term_bad[k] = 1;
    const uint32_t* r = rec + k * kWsumWeightWords;
    const uint32_t flags = r[8];
    good = good && (flags & kWsumValid) != 0;
    ok = ok && good;
    if (!good || (flags & kWsumZero) || c.inf) continue;
    GlvRecoded w;
    w.neg = w.u = 0;
    TC_UNROLL for (int i = 0; i < 4; i++) {
      w.neg |= (tc_u128)r[i] << (32 * i);
      w.u |= (tc_u128)r[4 + i] << (32 * i);
    }
    w.top = (flags & kWsumTop) != 0;
    w.flip = (flags & kWsumFlip) != 0;
    acc = jac_add(acc, g1_mul_glv_recoded(c, w));
  }
  return acc;
}

// out = sum_{k < n, included} w_k vals[k * term_stride] mod r  (`Poly * Fr` src/poly.rs:210-254 per coefficient, then :876).  w: n x 32 B
// LE canonical, shared by all outputs.  An included non-canonical value or weight: zero output, TC_JOB_INVALID_ENCODING.
TC_HD uint8_t job_fr_wsum(const uint8_t* vals, size_t term_stride, size_t n, const uint8_t* w_le32, const uint8_t* mask, uint8_t* out32) {
  Fr acc = Fr::zero();
  bool ok = true;
  TC_NOUNROLL for (size_t k = 0; k < n; k++) {
    if (mask && mask[k] == 0) continue;
    uint32_t v[8], w[8];
    const bool good = fr_from_le32(vals + k * term_stride, v) & fr_from_le32(w_le32 + k * 32, w);
    ok = ok && good;
    if (good) acc = acc + Fr::from_canonical(v) * Fr::from_canonical(w);
  }
  if (!ok) acc = Fr::zero();
  fr_store_le32(acc, out32);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

// Who deals into a resharing.  Plain integer code (host and device).  Part p is accepted when accept is null or accept[p] != 0
// and claims to be old node dealer_idx[p].  dup[p] = 1 for an accepted part whose index repeats that of an EARLIER accepted part
// (the first claim of an index is not marked).  S = the first t_old + 1 accepted parts in part order, the `take(t + 1)` of
// src/lib.rs:719-767: used[p] = 1 on S, sel_part / sel_idx (t_old + 1 entries each) = its part numbers and dealer indices in that
// order -- the abscissae of lagrange_all_at_zero are sel_idx + 1.  Returns false, with used all zero and nothing selected,
// when fewer than t_old + 1 parts are accepted; dup is filled in either way.  Any of used, sel_part, sel_idx, dup may be null.
TC_HD bool reshare_accepted(const uint8_t* accept, size_t p) { return !accept || accept[p] != 0; }
TC_HD bool reshare_is_duplicate(const uint8_t* accept, const uint64_t* dealer_idx, size_t p) {
  if (!reshare_accepted(accept, p)) return false;
  TC_NOUNROLL for (size_t q = 0; q < p; q++)
    if (reshare_accepted(accept, q) && dealer_idx[q] == dealer_idx[p]) return true;
  return false;
}
TC_HD bool reshare_select(const uint8_t* accept, const uint64_t* dealer_idx, size_t t_old, size_t P, uint8_t* used, uint32_t* sel_part,
                          uint64_t* sel_idx, uint8_t* dup) {
  size_t accepted = 0;
  TC_NOUNROLL for (size_t p = 0; p < P; p++) {
    if (dup) dup[p] = reshare_is_duplicate(accept, dealer_idx, p) ? 1 : 0;
    if (reshare_accepted(accept, p)) accepted++;
  }
  const bool enough = accepted > t_old;
  size_t taken = 0;
  TC_NOUNROLL for (size_t p = 0; p < P; p++) {
    const bool take = enough && taken <= t_old && reshare_accepted(accept, p);
    if (used) used[p] = take ? 1 : 0;
    if (take) {
      if (sel_part) sel_part[taken] = (uint32_t)p;
      if (sel_idx) sel_idx[taken] = dealer_idx[p];
      taken++;
    }
  }
  return enough;
}

// old_commit.evaluate(idx + 1) (src/poly.rs:497-508), the public key share old node idx is known to hold -- job_commitment_evaluate_at
// with the abscissa idx + 1 taken in Fr, so idx = 2^64 - 1 (abscissa 2^64: 64 doublings per Horner step) is an index like any other
TC_HD uint8_t job_commitment_evaluate_idx(const uint8_t* commit, size_t degree, uint64_t idx, G1Jac& res) {
  const uint64_t x = idx + 1;
  G1Affine c;
  bool ok = g1_decode_uncompressed(commit + degree * 96, c);
  res = G1Jac::from_affine(c);
  TC_NOUNROLL for (size_t kk = degree; kk-- > 0;) {
    G1Jac scaled;
    if (x != 0) {
      scaled = g1_mul_u64(res, x);
    } else {
      scaled = res;
      TC_NOUNROLL for (int b = 0; b < 64; b++) scaled = jac_dbl(scaled);
    }
    ok &= g1_decode_uncompressed(commit + kk * 96, c);
    res = jac_add_mixed(scaled, c);
  }
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
// the constant check of one dealer: its C[pos(0, 0)] (c0: 96 B) against old_commit.evaluate(idx + 1), as GROUP ELEMENTS (both
// sides re-encoded canonically).  OK / TC_JOB_SHARE_MISMATCH; INVALID_ENCODING when c0 does not decode.  An old_commit that does
// not decode is the caller's to notice (the answer is then meaningless).
TC_HD uint8_t job_reshare_constant_check(const uint8_t* old_commit, size_t t_old, uint64_t idx, const uint8_t* c0) {
  G1Jac want;
  (void)job_commitment_evaluate_idx(old_commit, t_old, idx, want);
  G1Affine got;
  if (!g1_decode_uncompressed(c0, got)) return TC_JOB_INVALID_ENCODING;
  uint8_t a[96], b[96];
  g1_encode_uncompressed(jac_to_affine(want), a);
  g1_encode_uncompressed(got, b);
  bool same = true;
  TC_NOUNROLL for (int i = 0; i < 96; i++) same = same && a[i] == b[i];
  return same ? TC_JOB_OK : TC_JOB_SHARE_MISMATCH;
}

}  // namespace tc
