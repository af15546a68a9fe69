// TEST HARNESS ONLY (tests/test_combine_quotient_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with
// g++ and exposes the quotient form of the [1 / D] step of the subset-grouped G2 combination: the decomposition, the job
// body with either divide form forced, the division alone, and the prediction that chooses.  Never linked into libtc_amd.so.
#include "tc_jobs.h"
#include <string.h>
using namespace tc;

extern "C" {
#if defined(TC_COUNT_OPS)
// mul2, split mul, split sqr, all mul, all sqr -- as tests/hostsim hs_op_counts5
void cq_op_counts5(uint64_t* out, int reset) {
  out[0] = g_tc_mul2_count;
  out[1] = g_tc_split_mul_count;
  out[2] = g_tc_split_sqr_count;
  out[3] = g_tc_mul_count;
  out[4] = g_tc_sqr_count;
  if (reset) g_tc_mul2_count = g_tc_split_mul_count = g_tc_split_sqr_count = g_tc_mul_count = g_tc_sqr_count = 0;
}
static uint64_t g_cq_divide_counts[5];
void cq_divide_counts5(uint64_t* out) { memcpy(out, g_cq_divide_counts, sizeof(g_cq_divide_counts)); }  // of the last cq_divide
// what one doubling (which = 0) and one mixed addition (1) of the ladders execute: run between two reads of the counters
void cq_one_step(int which, const uint8_t* pt) {
  G2Affine p;
  if (!g2_decode_uncompressed(pt, p)) return;
  G2Jac a = jac_dbl(G2Jac::from_affine(p));
  bool exc = false;
#if defined(TC_COUNT_OPS)
  g_tc_mul2_count = g_tc_split_mul_count = g_tc_split_sqr_count = g_tc_mul_count = g_tc_sqr_count = 0;
#endif
  a = which ? jac_add_mixed_generic(a, p, exc) : jac_dbl(a);
}
#endif
int cq_width() { return kQuotWidth; }
int cq_macs_dbl() { return (int)kMacsDbl; }
int cq_macs_add() { return (int)kMacsAdd; }
int cq_decompose(uint64_t D, uint64_t* q, int64_t* T, int64_t* E) { return combine_quotient_decompose(D, q, T, E) ? 1 : 0; }
int cq_small_coeffs(int t, const uint64_t* idx, uint64_t* c_abs, uint64_t* d_abs) {
  bool c_neg[4], d_neg;
  if (t == 1) return lagrange_small_coeffs<2>(idx, c_abs, c_neg, d_abs, &d_neg);
  if (t == 2) return lagrange_small_coeffs<3>(idx, c_abs, c_neg, d_abs, &d_neg);
  return lagrange_small_coeffs<4>(idx, c_abs, c_neg, d_abs, &d_neg);
}
// form = 0: the wave's own choice; 1: the 4-dimensional ladder; 2: the quotient form.  -1: not the fast path's
int cq_combine_g2(int t, const uint64_t* idx, const uint8_t* shares, uint8_t* out, int form) {
  g_tc_force_divide_form = form;
  uint8_t st = 0;
  bool done = false;
  if (t == 1) done = job_combine_small<Fq2, 2>(idx, shares, out, &st);
  if (t == 2) done = job_combine_small<Fq2, 3>(idx, shares, out, &st);
  if (t == 3) done = job_combine_small<Fq2, 4>(idx, shares, out, &st);
  g_tc_force_divide_form = 0;
  return done ? (int)st : -1;
}
// the choice for a generic D (1 = the quotient form) and the multiply-adds it predicts for the two forms (0: no decomposition)
int cq_choice(uint64_t D, uint32_t* uniform_macs, uint32_t* quotient_macs) {
  uint64_t q;
  int64_t T[4], E[4];
  *uniform_macs = combine_divide_uniform_macs(D);
  *quotient_macs = combine_quotient_decompose(D, &q, T, E) ? combine_divide_quotient_macs(q, T, E) : 0;
  return combine_divide_takes_quotient(D) ? 1 : 0;
}
// [1 / D] of an encoded point by one form alone (1 or 2), without the second pass of flagged lanes; returns the flag, -1 when the
// point does not decode or the form does not exist for D.  The counting build keeps the operations of the division itself.
int cq_divide(int form, uint64_t D, const uint8_t* pt, uint8_t* out) {
  G2Affine p;
  if (!g2_decode_uncompressed(pt, p)) return -1;
  uint64_t q;
  int64_t T[4], E[4];
  if (form == 2 && !combine_quotient_decompose(D, &q, T, E)) return -1;
  bool exc = false;
  // (a Z that is neither one nor real, as the short ladder leaves it)
  G2Jac a = jac_dbl(jac_add_mixed(jac_dbl(G2Jac::from_affine(p)), p));
#if defined(TC_COUNT_OPS)
  g_tc_mul2_count = g_tc_split_mul_count = g_tc_split_sqr_count = g_tc_mul_count = g_tc_sqr_count = 0;  // the division alone
#endif
  const G2Jac r = form == 2 ? combine_divide_quotient(a, D, exc) : combine_divide_uniform(a, D, exc);
#if defined(TC_COUNT_OPS)
  cq_op_counts5(g_cq_divide_counts, 1);
#endif
  g2_encode_uncompressed(jac_to_affine(r), out);
  return exc ? 1 : 0;
}
}
