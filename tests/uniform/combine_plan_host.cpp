// TEST HARNESS ONLY (tests/test_combine_plan_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with g++ and
// exposes the planned quotient form of the [1 / D] step of the subset-grouped G2 combination: the plan of a denominator, the
// multiply-adds it predicts, the division by a plan (the cheapest one or a forced one) and the job body.  Never linked into
// libtc_amd.so.
#include "tc_jobs.h"
#include <string.h>
using namespace tc;

extern "C" {
#if defined(TC_COUNT_OPS)
static uint64_t g_cp_divide_counts[5];
// mul2, split mul, split sqr, all mul, all sqr of the last cp_divide -- as tests/hostsim hs_op_counts5
void cp_divide_counts5(uint64_t* out) { memcpy(out, g_cp_divide_counts, sizeof(g_cp_divide_counts)); }
#endif
int cp_shift_lo() { return kQuotPlanShiftLo; }
int cp_shift_hi() { return kQuotPlanShiftHi; }
int cp_decompose(uint64_t D, uint64_t* q, int64_t* T, int64_t* E) { return combine_quotient_decompose(D, q, T, E) ? 1 : 0; }
int cp_small_coeffs(int t, const uint64_t* idx, uint64_t* c_abs, uint64_t* d_abs) {
  bool c_neg[4], d_neg;
  if (t == 1) return lagrange_small_coeffs<2>(idx, c_abs, c_neg, d_abs, &d_neg);
  if (t == 2) return lagrange_small_coeffs<3>(idx, c_abs, c_neg, d_abs, &d_neg);
  return lagrange_small_coeffs<4>(idx, c_abs, c_neg, d_abs, &d_neg);
}
// the plan of D: out = m, width, its multiply-adds, those of (m = 0, width 3) by combine_divide_quotient_macs, those of the
// 4-dimensional ladder.  force = 16 (m + 8) + width asks for that candidate's figures instead (0: the cheapest).  0: no decomposition
int cp_plan(uint64_t D, int force, int64_t* out) {
  uint64_t q;
  int64_t T[4], E[4];
  if (!combine_quotient_decompose(D, &q, T, E)) return 0;
  g_tc_force_quot_plan = force;
  const QuotPlan p = combine_quotient_plan(q, T, E);
  g_tc_force_quot_plan = 0;
  out[0] = p.m;
  out[1] = p.width;
  out[2] = p.macs;
  out[3] = combine_divide_quotient_macs(q, T, E);
  out[4] = combine_divide_uniform_macs(D);
  return 1;
}
// [1 / D] of an encoded point by the planned form alone (force as above), without the second pass of flagged lanes; returns the
// flag, -1 when the point does not decode or D has no decomposition.  The counting build keeps the operations of the division.
int cp_divide(uint64_t D, int force, const uint8_t* pt, uint8_t* out) {
  G2Affine p;
  if (!g2_decode_uncompressed(pt, p)) return -1;
  uint64_t q;
  int64_t T[4], E[4];
  if (!combine_quotient_decompose(D, &q, T, E)) return -1;
  bool exc = false;
  // (a Z that is neither one nor real, as the short ladder leaves it)
  G2Jac a = jac_dbl(jac_add_mixed(jac_dbl(G2Jac::from_affine(p)), p));
  g_tc_force_quot_plan = force;
#if defined(TC_COUNT_OPS)
  g_tc_mul2_count = g_tc_split_mul_count = g_tc_split_sqr_count = g_tc_mul_count = g_tc_sqr_count = 0;  // the division alone
#endif
  const G2Jac r = combine_divide_planned(a, q, T, E, combine_quotient_plan(q, T, E), exc);
#if defined(TC_COUNT_OPS)
  g_cp_divide_counts[0] = g_tc_mul2_count;
  g_cp_divide_counts[1] = g_tc_split_mul_count;
  g_cp_divide_counts[2] = g_tc_split_sqr_count;
  g_cp_divide_counts[3] = g_tc_mul_count;
  g_cp_divide_counts[4] = g_tc_sqr_count;
#endif
  g_tc_force_quot_plan = 0;
  g2_encode_uncompressed(jac_to_affine(r), out);
  return exc ? 1 : 0;
}
// the job body as a wave of one subset runs it (form = 0: the wave's own choice; 2: the planned quotient form wherever it exists);
// -1: not the fast path's
int cp_combine_g2(int t, const uint64_t* idx, const uint8_t* shares, uint8_t* out, int form, int force) {
  g_tc_force_divide_form = form;
  g_tc_force_quot_plan = force;
  uint8_t st = 0;
  bool done = false;
  if (t == 1) done = job_combine_small<Fq2, 2>(idx, shares, out, &st);
  if (t == 2) done = job_combine_small<Fq2, 3>(idx, shares, out, &st);
  if (t == 3) done = job_combine_small<Fq2, 4>(idx, shares, out, &st);
  g_tc_force_divide_form = 0;
  g_tc_force_quot_plan = 0;
  return done ? (int)st : -1;
}
}
