// Many scalars over ONE G1 point: the decryption shares of a ciphertext by its selected key holders
// (SecretKeyShare::decrypt_share_no_verify, /root/reference/src/lib.rs:460-462, once per holder) -- the G1 twin of
// tc_comb.h.  The base-4 sign-aligned GLV multiplication (tc_gls.h g1_mul_glv_ladder) is
//     [k'] P = 4^64 S + sum_{c < 64} 4^c sigma_c T[m_c],    T = { P, P - phi', P + 2 phi', P + phi', 3P, 3P + phi', 3P + 2 phi',
//                                                                 3P + 3 phi' },  phi' = [x^2] P,  S = P or P + phi',
// 128 doublings + 64 additions per scalar -- and the doublings do not depend on the scalar.  With enough scalars per point
// they are done ONCE, on the table:
//   stage T  one lane per ciphertext: column 0 of the comb is T itself (truly affine: two inversions), column c is FOUR times
//            column c-1 by two AFFINE doublings (lambda = 3 x^2 / 2 y), the eight inversions of a doubling shared
//            (Montgomery's trick); of column 64 only the two start entries are kept.  (64 x 8 + 2) entries x 128 B = 66 KB per
//            ciphertext, in HBM, in the G1 entry layout of tc_msm.h.
//   stage S  one lane per (ciphertext, kCombG1Share holders): per holder 64 MIXED additions  acc += +-comb[c][m_c]  onto the
//            start entry, no doubling, with the branch-free generic addition (tc_curve.h); the results share one inversion.
// The table is built over P, not over -P as the ladder's is for an even scalar: the RESULT is negated instead.  Same group
// elements, same bytes as the per-scalar ladders.
#pragma once
#include "tc_msm.h"

namespace tc {

constexpr int kCombG1Columns = 64;                                               // digit columns 0 .. 63 of eight entries each
constexpr int kCombG1Entries = kCombG1Columns * 8 + 2;                           // + the start entries 4^64 P, 4^64 (P + phi')
constexpr int kCombG1TableWords = kCombG1Entries * kMsmEntryWordsG1;             // per ciphertext
constexpr int kCombG1Share = 8;                                                  // holders per lane in stage S

#if defined(TC_COMB_G1_COUNT) && !defined(__HIPCC__)
inline unsigned long tc_comb_g1_fallbacks = 0;  // host test build: holders whose multiplication took the guarded fallback
#endif

// Stage T.  false: u does not decode (every entry is then the identity and stage S fails the ciphertext's shares).  The identity
// as u is a valid operand: every entry at infinity, true.
TC_HD bool job_comb_tables_g1(const uint8_t* u96, int32_t* tbl) {
  G1Affine p;
  const bool ok = g1_decode_uncompressed(u96, p);
  if (!ok) p = G1Affine::infinity();
  G1Affine e[8];
  {
    // 2P, 3P, then the six proper sums: the entries and their order are those of g1_mul_glv_ladder's table
    G1Jac mult[2];
    mult[0] = jac_dbl(G1Jac::from_affine(p));
    mult[1] = jac_add_mixed(mult[0], p);
    G1Affine ma[2];
    jac_batch_to_affine<Fq, 2>(mult, ma, 2);
    const G1Affine p2 = ma[0], p3 = ma[1];
    G1Affine f1 = g1_phi(p), f2 = g1_phi(p2), f3 = g1_phi(p3);  // phi' = -phi: negate y below
    const G1Affine m1 = f1;                                    // -phi'(P) = phi(P)
    f1.y = (-f1.y).norm();
    f2.y = (-f2.y).norm();
    f3.y = (-f3.y).norm();
    G1Jac sums[6];
    sums[0] = jac_add_affine(p, m1);   // 1: P - phi'
    sums[1] = jac_add_affine(p, f2);   // 2: P + 2 phi'
    sums[2] = jac_add_affine(p, f1);   // 3: P + phi'
    sums[3] = jac_add_affine(p3, f1);  // 5: 3P + phi'
    sums[4] = jac_add_affine(p3, f2);  // 6: 3P + 2 phi'
    sums[5] = jac_add_affine(p3, f3);  // 7: 3P + 3 phi'
    G1Affine aff[6];
    jac_batch_to_affine<Fq, 6>(sums, aff, 6);
    e[0] = p;
    e[4] = p3;
    TC_UNROLL for (int m = 0; m < 3; m++) {
      e[1 + m] = aff[m];
      e[5 + m] = aff[3 + m];
    }
  }
  TC_NOUNROLL for (int m = 0; m < 8; m++) {
    e[m].x = e[m].x.norm();
    e[m].y = e[m].y.norm();
    msm_store_entry_g1(tbl + m * kMsmEntryWordsG1, e[m]);
  }
  TC_NOUNROLL for (int c = 1; c <= kCombG1Columns; c++) {
    tc_fair();
    TC_NOUNROLL for (int half = 0; half < 2; half++) {
      // 1 / (2 y) of the eight entries with one inversion (an entry at infinity counts as 1 and stays at infinity; 2 y = 0
      // needs a point of order two, which E(Fq) does not have: its cofactor is odd)
      Fq pre[8];
      Fq acc = Fq::one();
      TC_NOUNROLL for (int m = 0; m < 8; m++) {
        pre[m] = acc;
        acc = acc * Fq::select(e[m].inf, Fq::one(), e[m].y.dbl());
      }
      Fq inv = acc.inv();
      TC_NOUNROLL for (int m = 7; m >= 0; m--) {
        const Fq d = Fq::select(e[m].inf, Fq::one(), e[m].y.dbl());
        const Fq di = inv * pre[m];
        inv = inv * d;
        const Fq xx = e[m].x.sqr();
        const Fq lam = ((xx.dbl() + xx).norm()) * di;            // 3 x^2 / (2 y)
        // (x3 = lambda^2 - 2 x feeds its own value back doubled: pull it to ~p every doubling, tc_field.h reduce_value)
        const Fq x3 = (lam.sqr() - e[m].x.dbl()).reduce_value();
        const Fq y3 = (lam * (e[m].x - x3) - e[m].y).reduce_value();
        e[m].x = x3;
        e[m].y = y3;
      }
    }
    if (c < kCombG1Columns) {
      TC_NOUNROLL for (int m = 0; m < 8; m++) msm_store_entry_g1(tbl + (size_t)(c * 8 + m) * kMsmEntryWordsG1, e[m]);
    } else {
      msm_store_entry_g1(tbl + (size_t)(kCombG1Columns * 8) * kMsmEntryWordsG1, e[0]);
      msm_store_entry_g1(tbl + (size_t)(kCombG1Columns * 8 + 1) * kMsmEntryWordsG1, e[3]);
    }
  }
  return ok;
}

// Stage S: out[s] = sk[idx[s]] * P for n <= kCombG1Share holder indices into a table of N secret key shares, from the
// ciphertext's comb.  An index >= N or a scalar >= r fails its own output, an undecodable u (table_ok = false) all n.  The
// recoded digits stay in registers.  A lane that takes fewer holders than its wave's longest one repeats its first and drops
// the result: the loop is the wave's.
TC_HD void job_comb_decrypt(const uint8_t* sk_table, size_t N, const uint64_t* idx, int n, const int32_t* tbl, bool table_ok, uint8_t* out,
                            uint8_t* status) {
  G1Jac res[kCombG1Share];
  bool ok[kCombG1Share];
  TC_NOUNROLL for (int s = 0; wave_any(s < n); s++) {
    const bool live = s < n;
    uint32_t k[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t i = idx[live ? s : 0];
    bool good = table_ok && i < N;
    if (i < N) good = fr_from_le32(sk_table + 32 * i, k) && good;
    if (!good) {  // (validity is public: a rejected holder multiplies by one and drops the result)
      TC_UNROLL for (int w = 0; w < 8; w++) k[w] = (w == 0) ? 1u : 0u;
    }
    tc_u128 neg, u;
    bool top;
    const bool flip = glv_recode_sign_aligned(k, &neg, &u, &top);
    const G1Affine start = msm_load_entry_g1(tbl + (size_t)(kCombG1Columns * 8 + (top ? 1 : 0)) * kMsmEntryWordsG1);
    G1Jac acc = G1Jac{start.x, start.y, Fq::one()};
    bool exc = start.inf;
    TC_NOUNROLL for (int c = kCombG1Columns - 1; c >= 0; c--) {
      if ((c & 15) == 15) tc_fair();
      const uint32_t nn = (uint32_t)(neg >> 126) & 3u, w = (uint32_t)(u >> 126) & 3u;  // bit 1: column 2c+1, bit 0: column 2c
      neg <<= 2;
      u <<= 2;
      const bool sub = (nn >> 1) != 0;
      const uint32_t m = w | ((((nn >> 1) ^ nn) & 1u) ? 0u : 4u);
      G1Affine e = msm_load_entry_g1(tbl + (size_t)(c * 8 + (int)m) * kMsmEntryWordsG1);
      e.y = Fq::select(sub, -e.y, e.y);
      acc = jac_add_mixed_generic(acc, e, exc);
    }
    acc.y = Fq::select(flip, -acc.y, acc.y);  // the comb is built over P, the ladder's table over -P: negate the result
    if (wave_any(exc)) {
      // a lane that may have met a special case (u at infinity, a partial sum that met +-its entry: k = 0): the guarded ladder
      // on the decoded point, column 0's first entry
      const G1Affine p = msm_load_entry_g1(tbl);
      acc = G1Jac::select(exc, g1_mul_glv(p, k), acc);
#if defined(TC_COMB_G1_COUNT) && !defined(__HIPCC__)
      if (exc) tc_comb_g1_fallbacks++;
#endif
    }
    if (live) {
      ok[s] = good;
      res[s] = G1Jac::select(good, acc, G1Jac::infinity());
    }
  }
  G1Affine aff[kCombG1Share];
  jac_batch_to_affine<Fq, kCombG1Share>(res, aff, n);
  TC_NOUNROLL for (int s = 0; s < n; s++) {
    g1_encode_uncompressed(aff[s], out + (size_t)s * 96);
    if (status) status[s] = ok[s] ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  }
}

// The form for few holders or small batches: one ladder per (ciphertext, selected holder), the scalar gathered through idx
// (the table of the ladder in the wave's arena slot, as k_g1_mul_arena keeps it: every lane of the wave runs the ladder).
TC_HD uint8_t job_g1_mul_gather(const uint8_t* sk_table, size_t N, uint64_t i, const uint8_t* pt, uint8_t* out) {
  uint32_t k[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  G1Affine p;
  bool ok = i < N;
  if (i < N) ok = fr_from_le32(sk_table + 32 * i, k);
  ok &= g1_decode_uncompressed(pt, p);
  if (!ok) {
    p = G1Affine{g1_generator().x, g1_generator().y, true};
    TC_UNROLL for (int w = 0; w < 8; w++) k[w] = (w == 0) ? 1u : 0u;
  }
  const G1Affine r = jac_to_affine(g1_mul_glv_arena(p, k));
  g1_encode_uncompressed(ok ? r : G1Affine::infinity(), out);
  return ok ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}

}  // namespace tc
