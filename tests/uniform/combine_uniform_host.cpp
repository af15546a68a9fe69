// TEST HARNESS ONLY (tests/test_combine_uniform_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with
// g++ and exposes the pieces of the subset-grouped G2 combination: the two recodings, the job body in its wave-uniform
// and its mixed-wave form, psi^2 at the table look-up, and the grouping plan.  Never linked into libtc_amd.so.
#include "tc_jobs.h"
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
#if defined(TC_COUNT_OPS)
// mul2 (Fq2 products' coefficient formulas), split mul, split sqr, all mul, all sqr -- as tests/hostsim hs_op_counts5
void cu_op_counts5(uint64_t* out, int reset) {
  out[0] = g_tc_mul2_count;
  out[1] = g_tc_split_mul_count;
  out[2] = g_tc_split_sqr_count;
  out[3] = g_tc_mul_count;
  out[4] = g_tc_sqr_count;
  if (reset) g_tc_mul2_count = g_tc_split_mul_count = g_tc_split_sqr_count = g_tc_mul_count = g_tc_sqr_count = 0;
}
#endif
int cu_wnaf_cols() { return kWnafCols; }
void cu_wnaf4(uint64_t d, int8_t* dig) { wnaf4_recode(d, dig); }
void cu_naf(uint64_t c, uint64_t* pos, uint64_t* neg) { naf_recode(c, pos, neg); }
// the small integers of the fast path; 0 when it does not take the tuple
int cu_small_coeffs(int t, const uint64_t* idx, uint64_t* c_abs, uint64_t* d_abs) {
  bool c_neg[4], d_neg;
  if (t == 1) return lagrange_small_coeffs<2>(idx, c_abs, c_neg, d_abs, &d_neg);
  if (t == 2) return lagrange_small_coeffs<3>(idx, c_abs, c_neg, d_abs, &d_neg);
  return lagrange_small_coeffs<4>(idx, c_abs, c_neg, d_abs, &d_neg);
}
// the four base-|x| digits of D^-1 mod r
void cu_inverse_digits(uint64_t d_abs, uint64_t* d) {
  uint32_t dinv[8];
  fr_inverse_of_small(d_abs, false, dinv);
  gls_decompose(dinv, d);
}
// mixed = 0: the wave-uniform forms (on the host one job is a wave); 1: the forms of a mixed wave.  -1: not the fast path's
int cu_combine_g2(int t, const uint64_t* idx, const uint8_t* shares, uint8_t* out, int mixed) {
  g_tc_force_mixed_combine = mixed;
  uint8_t st = 0;
  bool done = false;
  if (t == 1) done = job_combine_small<Fq2, 2>(idx, shares, out, &st);
  if (t == 2) done = job_combine_small<Fq2, 3>(idx, shares, out, &st);
  if (t == 3) done = job_combine_small<Fq2, 4>(idx, shares, out, &st);
  g_tc_force_mixed_combine = 0;
  return done ? (int)st : -1;
}
// psi(psi(P)) against (PSI2_CX x, -y), both encoded
int cu_psi2(const uint8_t* pt, uint8_t* by_psi, uint8_t* by_constant) {
  G2Affine p;
  if (!g2_decode_uncompressed(pt, p)) return -1;
  g2_encode_uncompressed(g2_psi(g2_psi(p)), by_psi);
  const G2Affine q{p.x.scale(Fq::from_limbs(PSI2_CX)), (-p.y).norm(), p.inf};
  g2_encode_uncompressed(q, by_constant);
  return 0;
}
uint32_t cu_group_slots(size_t B) { return (uint32_t)(B + (size_t)kSubsetMaxGroups * (kSubsetPad - 1)); }
// The grouping of B jobs as k_combine_keys / k_combine_plan / k_combine_place build it, one job after the other: the keys
// and the plan come from the shared functions of tc_jobs.h.  perm: cu_group_slots(B) words.  Returns the mode (1 = subset),
// -1 when a position falls outside perm; *groups = distinct keys seen before the table overflowed.
int cu_plan(int t, const uint64_t* idx, size_t n_per_job, size_t B, uint32_t* perm, uint32_t* starts, uint8_t* orders, uint32_t* groups) {
  std::vector<uint64_t> keys(kSubsetSlots, 0);
  std::vector<uint32_t> count(kSubsetSlots, 0), rank(B, 0), crank(B, 0), grp(B, 0);
  std::vector<uint8_t> order(kSubsetSlots, kGroupOrders - 1), cls(B, 0);
  uint32_t ccount[kCombineClasses] = {0, 0, 0}, ngroups = 0;
  bool overflow = false;
  for (size_t j = 0; j < B; j++) {
    int c;
    const uint64_t key = combine_tuple_key(idx + j * n_per_job, t, &c);
    cls[j] = (uint8_t)c;
    crank[j] = ccount[c]++;
    if (overflow) continue;
    uint32_t h = combine_key_hash(key) & (kSubsetSlots - 1);
    bool found = false;
    for (uint32_t probe = 0; probe < kSubsetSlots && !found; probe++) {
      if (keys[h] == 0) {
        keys[h] = key;
        if (ngroups++ >= kSubsetMaxGroups) overflow = true;
      }
      if (keys[h] == key) found = true;
      else h = (h + 1) & (kSubsetSlots - 1);
    }
    if (!found) {
      overflow = true;
      continue;
    }
    grp[j] = h;
    rank[j] = count[h]++;
  }
  *groups = ngroups;
  for (uint32_t s = 0; s < kSubsetSlots; s++)
    if (keys[s]) order[s] = (uint8_t)combine_key_order(keys[s], t);
  const bool subset = combine_subset_mode(overflow, ngroups, B);
  uint8_t corder[kCombineClasses];
  uint32_t cstart[kCombineClasses];
  for (int c = 0; c < kCombineClasses; c++) corder[c] = (uint8_t)combine_class_order(c);
  for (int c = 0; c < kCombineClasses; c++) cstart[c] = combine_group_start(ccount, corder, kCombineClasses, (uint32_t)c, kClassPad);
  const size_t slots = cu_group_slots(B);
  memset(perm, 0xff, slots * sizeof(uint32_t));
  for (uint32_t s = 0; s < kSubsetSlots; s++) {
    starts[s] = subset && count[s] ? combine_group_start(count.data(), order.data(), kSubsetSlots, s, kSubsetPad) : 0xffffffffu;
    orders[s] = order[s];
  }
  for (size_t j = 0; j < B; j++) {
    const size_t pos = subset ? (size_t)combine_group_start(count.data(), order.data(), kSubsetSlots, grp[j], kSubsetPad) + rank[j]
                              : (size_t)cstart[cls[j]] + crank[j];
    if (pos >= slots) return -1;
    perm[pos] = (uint32_t)j;
  }
  return subset ? 1 : 0;
}
}
