// Host leg of the DKG kernel conformance harness (tests/dkg_conformance.py): the header routines the kernels of k_dkg.hip call
// (tc_dkg.h) -- fixed_base_table_entry, job_g1_fixed_base_mul, job_bivar_commitment_row, job_commitment_evaluate_at,
// job_fr_interpolate, the Montgomery conversions, job_fr_poly_evaluate, job_bivar_poly_row, job_fr_sum / _wsum,
// job_fr_interpolate_at_zero, job_g1_sum_part, wsum_recode_weight, job_g1_wsum_part, dkg_rlc_scalar, job_reshare_constant_check and
// the resharing verdict chain -- run by g++ with -DTC_BOUND_CHECK over the same buffers, in the layout of tests/device/dkg_kernels.hip:
// the jobs one after the other, the lanes of an output one after the other, then the kernel's xor tree of jac_add.  It proves the
// case tables, the models and the checkers before any GPU time is spent.  What it cannot see is the kernels' own text (lane pairs,
// the shuffle merge, the indexing, the launch geometry): that is the GPU leg.  parts / slices = 0 (the launcher's rule) exist on
// the device only; the word-copy kernels and the two comparisons have no header routine and no entry here.
// With -DDK_MAIN it is a stand-alone program over a short fixed case list (for a g++ -fsanitize=address,undefined build).
// Test code only: never linked into libtc_amd.so.
#include "../../threshold_crypto_amd/csrc/tc_dkg.h"

#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tc;

namespace {
const int32_t* fb_table() {
  static std::vector<int32_t> tbl;
  if (tbl.empty()) {
    tbl.resize(kFbTableWords);
    for (int e = 0; e < kFbWindows * kFbEntries; e++) fixed_base_table_entry(e, tbl.data() + (size_t)e * kFbPointWords);
  }
  return tbl.data();
}
struct Lane {
  G1Jac r;
  int good;
};
// the kernels' merge: every lane adds its partner's value of the round before, the validity flags travel with the sums
Lane merge(std::vector<Lane> r, size_t parts) {
  for (size_t d = 1; d < parts; d <<= 1) {
    std::vector<Lane> nr(parts);
    for (size_t g = 0; g < parts; g++) nr[g] = Lane{jac_add(r[g].r, r[g ^ d].r), r[g].good & r[g ^ d].good};
    r = nr;
  }
  return r[0];
}
size_t legal_parts(size_t parts) { return (parts < 1 || parts > 64 || (parts & (parts - 1))) ? 1 : parts; }
size_t term0(int column0, size_t j) { return (column0 ? bivar_coeff_pos(j, 0) : j) * 96; }
}  // namespace

extern "C" {
int dkh_fixed_base_table(int32_t* tbl) {
  memcpy(tbl, fb_table(), (size_t)kFbTableWords * sizeof(int32_t));
  return 0;
}
int dkh_g1_fixed_base(const uint8_t* fr, size_t M, int cus, int with_status, uint8_t* out, uint8_t* status) {
  for (size_t j = 0; j < M; j++) {
    const uint8_t st = job_g1_fixed_base_mul(fb_table(), fr + j * 32, out + j * 96);
    if (with_status) status[j] = st;
  }
  return 0;
}
int dkh_commitment_rows(int form, const uint8_t* commits, size_t commit_bytes, size_t stride, size_t degree, const uint64_t* xs, size_t B, size_t n,
                        int with_status, uint8_t* out, uint8_t* status) {
  if (form < 0 || form > 2 || (form && !with_status)) return 1;
  const size_t per = degree + 1, lanes = form == 2 ? B * n : B * per;
  for (size_t t = 0; t < lanes; t++) {
    uint8_t st;
    if (form == 0) st = job_bivar_commitment_row(commits, degree, t % per, xs[t / per], out + t * 96);
    else if (form == 1) st = job_bivar_commitment_row(commits + (t / per) * stride, degree, t % per, xs[t / per], out + t * 96);
    else st = job_commitment_evaluate_at(commits + (t / n) * per * 96, degree, xs[t], out + t * 96);
    if (with_status) status[t] = st;
  }
  return 0;
}
int dkh_fr_interpolate(size_t n, const uint32_t* xs, const uint32_t* ys, size_t B, int with_status, uint32_t* out, uint32_t* ws, uint8_t* status) {
  for (size_t j = 0; j < B; j++) {
    const uint8_t st = job_fr_interpolate(n, xs + j * n * 8, ys + j * n * 8, out + j * n * 8, ws + j * 2 * (n + 1) * 8);
    if (with_status) status[j] = st;
  }
  return 0;
}
int dkh_fr_interpolate_at_zero(size_t n, const uint64_t* xs, const uint8_t* vals, const uint8_t* accept, size_t P, uint8_t* out, uint8_t* status) {
  for (size_t p = 0; p < P; p++) {
    if (accept && accept[p] == 0) {
      memset(out + p * 32, 0, 32);
      status[p] = TC_JOB_OK;
    } else {
      status[p] = job_fr_interpolate_at_zero(n, xs + p * n, vals + p * n * 32, out + p * 32);
    }
  }
  return 0;
}
int dkh_to_mont(const uint8_t* fr, size_t fr_bytes, size_t count, int degree, uint32_t* mont, uint8_t* valid) {
  if (degree >= 0 && count != (size_t)(degree + 1) * (degree + 1)) return 1;
  const size_t n = (size_t)degree + 1;
  for (size_t t = 0; t < count; t++)
    valid[t] = fr_mont_from_le32(fr + (degree < 0 ? t : bivar_coeff_pos(t / n, t % n)) * 32, mont + t * 8) ? 1 : 0;
  return 0;
}
int dkh_fr_poly_evaluate(const uint8_t* coeff, size_t n, const uint8_t* xs, size_t M, size_t B, int with_status, uint8_t* out, uint8_t* status) {
  std::vector<uint32_t> mont(B * n * 8 + 1);
  std::vector<uint8_t> valid(B * n + 1);
  for (size_t t = 0; t < B * n; t++) valid[t] = fr_mont_from_le32(coeff + t * 32, mont.data() + t * 8) ? 1 : 0;
  for (size_t t = 0; t < B * M; t++) {
    const size_t j = t / M, m = t % M;
    const uint8_t st = job_fr_poly_evaluate(mont.data() + j * n * 8, valid.data() + j * n, n, xs + m * 32, out + t * 32);
    if (with_status) status[t] = st;
  }
  return 0;
}
int dkh_bivar_poly_row(const uint8_t* coeff, size_t degree, const uint64_t* xs, size_t M, int with_status, uint8_t* out, uint8_t* status) {
  const size_t n = degree + 1;
  std::vector<uint32_t> mont(n * n * 8);
  std::vector<uint8_t> valid(n * n);
  for (size_t t = 0; t < n * n; t++) valid[t] = fr_mont_from_le32(coeff + bivar_coeff_pos(t / n, t % n) * 32, mont.data() + t * 8) ? 1 : 0;
  for (size_t t = 0; t < M * n; t++) {
    const uint8_t st = job_bivar_poly_row(mont.data(), valid.data(), degree, t % n, xs[t / n], out + t * 32);
    if (with_status) status[t] = st;
  }
  return 0;
}
int dkh_fr_sum(const uint8_t* vals, size_t vals_bytes, size_t term_stride, size_t n, const uint8_t* weights, const uint8_t* mask, size_t B,
               int with_status, uint8_t* out, uint8_t* status) {
  for (size_t j = 0; j < B; j++) {
    const uint8_t st = weights ? job_fr_wsum(vals + j * 32, term_stride, n, weights, mask, out + j * 32)
                               : job_fr_sum(vals + j * 32, term_stride, n, mask, out + j * 32);
    if (with_status) status[j] = st;
  }
  return 0;
}
int dkh_g1_sum(int column0, const uint8_t* pts, size_t pts_bytes, size_t term_stride, size_t n, const uint8_t* mask, const uint8_t* member, size_t B,
               size_t parts, int cus, int with_status, int with_term_bad, uint8_t* out, uint8_t* status, uint8_t* term_bad, size_t* used) {
  if (!parts) return 1;  // (the launcher's rule: the device leg only)
  used[0] = parts;
  parts = legal_parts(parts);
  if (with_term_bad) memset(term_bad, 0, n);
  for (size_t j = 0; j < B; j++) {
    std::vector<Lane> r(parts);
    for (size_t g = 0; g < parts; g++) {
      bool ok;
      r[g].r = job_g1_sum_part(pts + term0(column0, j), term_stride, mask, member ? member + j : nullptr, B, sum_part(n, g, parts), ok,
                               with_term_bad ? term_bad : nullptr);
      r[g].good = ok ? 1 : 0;
    }
    const Lane m = merge(r, parts);
    g1_encode_uncompressed(m.good ? jac_to_affine(m.r) : G1Affine::infinity(), out + j * 96);
    if (with_status) status[j] = m.good ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  }
  return 0;
}
int dkh_g1_wsum(int column0, const uint8_t* pts, size_t pts_bytes, size_t term_stride, size_t n_terms, const uint8_t* weights, size_t n,
                const uint8_t* mask, const uint8_t* member, size_t B, size_t parts, size_t slices, int cus, const uint32_t* sel, int chain, size_t rows,
                uint32_t* rec, uint8_t* out, uint8_t* status, uint8_t* part_ok, uint8_t* final_out, uint8_t* final_status, size_t* used) {
  if (!parts || !slices) return 1;  // (the launcher's rules: the device leg only)
  used[0] = parts;
  used[1] = slices > n ? n : slices;  // g1_wsum_slices' clamp of a forced value
  if (used[1] < 1) used[1] = 1;
  slices = used[1];
  if (B * slices > rows || (!sel && n != n_terms)) return 1;
  parts = legal_parts(parts);
  for (size_t k = 0; k < n_terms; k++) wsum_recode_weight(weights + k * 32, rec + k * kWsumWeightWords);
  for (size_t q = 0; q < B * slices; q++) {
    const size_t s = q / B, j = q % B;
    std::vector<Lane> r(parts);
    for (size_t g = 0; g < parts; g++) {
      bool ok;
      r[g].r = job_g1_wsum_part(pts + term0(column0, j), term_stride, rec, mask, member ? member + j : nullptr, B, wsum_slice_part(n, s, slices, g, parts),
                                ok, nullptr, sel);
      r[g].good = ok ? 1 : 0;
    }
    const Lane m = merge(r, parts);
    g1_encode_uncompressed(m.good ? jac_to_affine(m.r) : G1Affine::infinity(), out + q * 96);
    if (slices > 1) part_ok[q] = m.good ? 1 : 0;
    else status[q] = m.good ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
  }
  if (chain && slices > 1) {
    size_t u;
    return dkh_g1_sum(0, out, B * slices * 96, B * 96, slices, nullptr, part_ok, B, 1, cus, 1, 0, final_out, final_status, nullptr, &u);
  }
  return 0;
}
int dkh_rlc_scalars(const uint8_t* seed32, const uint64_t* xs, const uint8_t* vals, size_t n, size_t degree, size_t B, uint32_t* scalars,
                    uint8_t* valid) {
  uint32_t key[8];
  for (int w = 0; w < 8; w++)
    key[w] = (uint32_t)seed32[4 * w] | ((uint32_t)seed32[4 * w + 1] << 8) | ((uint32_t)seed32[4 * w + 2] << 16) | ((uint32_t)seed32[4 * w + 3] << 24);
  for (size_t j = 0; j < B; j++)
    valid[j] = job_dkg_rlc_scalars(key, j, n, degree, xs + j * n, vals + j * n * 32, scalars + j * (degree + 2) * 8) ? 1 : 0;
  return 0;
}
// the lanes of k_reshare_check, k_reshare_part_status, k_reshare_plan and k_reshare_guard one after the other
int dkh_reshare_chain(const uint8_t* old_commit, const uint8_t* old_member, size_t t_old, const uint64_t* dealer_idx, const uint8_t* commits,
                      size_t commit_bytes, size_t stride, size_t degree, const uint8_t* accept, const uint8_t* member, const uint8_t* share_st, size_t P,
                      uint8_t* const_st, uint8_t* point_bad, uint8_t* dup, uint8_t* old_bad, uint8_t* part_status, uint8_t* used, uint32_t* sel_part,
                      uint64_t* sel_idx, uint32_t* ws, uint8_t* weights, uint8_t* status, uint8_t* out_commit, uint8_t* out_share) {
  if (!P) return 1;
  memset(weights, 0, P * 32);
  bool bad = false;
  for (size_t k = 0; k <= t_old; k++) {
    G1Affine c;
    bad = bad || !g1_decode_uncompressed(old_commit + k * 96, c) || (old_member && old_member[k] == 0);
  }
  old_bad[0] = bad ? 1 : 0;
  for (size_t p = 0; p < P; p++) {
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
  for (size_t p = 0; p < P; p++) {
    uint8_t st = TC_JOB_OK;
    if (old_bad[0] == 0 && reshare_accepted(accept, p)) {
      const uint8_t ss = share_st ? share_st[p] : (uint8_t)TC_JOB_OK;
      if (point_bad[p] || const_st[p] == TC_JOB_INVALID_ENCODING || ss == TC_JOB_INVALID_ENCODING) st = TC_JOB_INVALID_ENCODING;
      else if (dup[p] || ss == TC_JOB_DUPLICATE_ENTRY) st = TC_JOB_DUPLICATE_ENTRY;
      else if (const_st[p] == TC_JOB_SHARE_MISMATCH) st = TC_JOB_SHARE_MISMATCH;
    }
    part_status[p] = st;
  }
  uint8_t st = old_bad[0] ? (uint8_t)TC_JOB_INVALID_ENCODING : (uint8_t)TC_JOB_OK;
  for (size_t p = 0; p < P && st == TC_JOB_OK; p++) st = part_status[p];
  bool selected = false;
  if (st == TC_JOB_OK) {
    selected = reshare_select(accept, dealer_idx, t_old, P, used, sel_part, sel_idx, nullptr);
    if (!selected) st = TC_JOB_NOT_ENOUGH_SHARES;
  }
  if (selected) {
    uint32_t* lam = ws;
    st = lagrange_all_at_zero(sel_idx, (int)t_old, lam, ws + (t_old + 1) * 8);
    if (st == TC_JOB_OK)
      for (size_t i = 0; i <= t_old; i++)
        for (int b = 0; b < 32; b++) weights[(size_t)sel_part[i] * 32 + b] = (uint8_t)(lam[i * 8 + (b >> 2)] >> (8 * (b & 3)));
  }
  if (st != TC_JOB_OK) memset(used, 0, P);
  status[0] = st;
  if (st != TC_JOB_OK) {
    for (size_t i = 0; i <= degree && out_commit; i++) g1_encode_uncompressed(G1Affine::infinity(), out_commit + i * 96);
    if (out_share) memset(out_share, 0, 32);
  }
  return 0;
}
void dkh_sum_part(size_t n, size_t s, size_t slices, size_t g, size_t parts, size_t* out2) {
  const SumPart p = slices ? wsum_slice_part(n, s, slices, g, parts) : sum_part(n, g, parts);
  out2[0] = p.k0;
  out2[1] = p.k1;
}
}

#if defined(DK_MAIN)
static void le32(uint64_t v, uint8_t* out) {
  memset(out, 0, 32);
  for (int b = 0; b < 8; b++) out[b] = (uint8_t)(v >> (8 * b));
}
static void gen_mul(uint64_t k, uint8_t* out96) { g1_encode_uncompressed(jac_to_affine(g1_mul_u64(G1Jac::from_affine(g1_generator()), k)), out96); }
static bool poison(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (p[i] != 0x5A) return false;
  return true;
}
int main() {
  int rc = 0, seen = 0;
  auto mark = [&](const char* what) {
    if (rc != seen) printf("dkg_kernels_host: %s failed\n", what);
    seen = rc;
  };
  // fixed base: 0, 1, 16 + 15 (a carry), 2^64 - 1 against the 64-bit ladder; a value >= r
  {
    const size_t M = 5;
    const uint64_t k[M] = {0, 1, 31, ~0ull, 0};
    std::vector<uint8_t> fr(M * 32), out((M + 1) * 96, 0x5A), st(M + 1, 0x5A), want(96);
    for (size_t j = 0; j < M; j++) le32(k[j], fr.data() + j * 32);
    memset(fr.data() + 4 * 32, 0xff, 32);
    rc |= dkh_g1_fixed_base(fr.data(), M, 1, 1, out.data(), st.data());
    for (size_t j = 0; j < 4; j++) {
      gen_mul(k[j], want.data());
      rc |= (memcmp(want.data(), out.data() + j * 96, 96) == 0 && st[j] == TC_JOB_OK) ? 0 : 1;
    }
    rc |= (st[4] == TC_JOB_INVALID_ENCODING && out[4 * 96] == 0x40 && poison(out.data() + M * 96, 96) && st[M] == 0x5A) ? 0 : 1;
  }
  mark("fixed base");
  // a commitment of degree 2 with coefficient (i, j) = (1 + pos) g1: rows at x = 0, 3, 2^64 - 1 in the three forms agree
  {
    const size_t deg = 2, n = deg + 1, B = 3;
    std::vector<uint8_t> c(6 * 96), row((B * n + 1) * 96, 0x5A), rowj((B * n + 1) * 96, 0x5A), st(B * n + 1, 0x5A), cj(B * 7 * 96, 0x11);
    for (size_t e = 0; e < 6; e++) gen_mul(e + 1, c.data() + e * 96);
    const uint64_t xs[B] = {0, 3, ~0ull};
    rc |= dkh_commitment_rows(0, c.data(), c.size(), 0, deg, xs, B, 0, 1, row.data(), st.data());
    for (size_t j = 0; j < B; j++) memcpy(cj.data() + j * 7 * 96, c.data(), 6 * 96);
    rc |= dkh_commitment_rows(1, cj.data(), cj.size(), 7 * 96, deg, xs, B, 0, 1, rowj.data(), st.data());
    rc |= memcmp(row.data(), rowj.data(), row.size()) ? 1 : 0;
    std::vector<uint8_t> want(96), ev((B + 1) * 96, 0x5A);
    gen_mul(2 + 3 * 3 + 5 * 9, want.data());  // row(3)[1] = c(1,0) + 3 c(1,1) + 9 c(1,2)
    rc |= memcmp(want.data(), row.data() + (1 * n + 1) * 96, 96) ? 1 : 0;
    // evaluate row(3) at 2 = sum_i row(3)[i] 2^i against the symmetric evaluation row(2) at 3
    std::vector<uint8_t> r3(n * 96 * B);
    for (size_t j = 0; j < B; j++) memcpy(r3.data() + j * n * 96, row.data() + 1 * n * 96, n * 96);
    const uint64_t at[B] = {2, 2, 2};
    rc |= dkh_commitment_rows(2, r3.data(), r3.size(), 0, deg, at, B, 1, 1, ev.data(), st.data());
    gen_mul((1 + 2 * 3 + 4 * 9) + 2 * (2 + 3 * 3 + 5 * 9) + 4 * (4 + 5 * 3 + 6 * 9), want.data());
    rc |= (memcmp(want.data(), ev.data(), 96) == 0 && poison(ev.data() + B * 96, 96)) ? 0 : 1;
  }
  mark("commitment rows");
  // interpolation through (1, 3), (2, 5), (4, 9): 1 + 2 X; a repeated abscissa; the workspace of job j + 1 behind job j's
  {
    const size_t n = 3, B = 2, blk = 2 * (n + 1) * 8;
    std::vector<uint32_t> xs(B * n * 8, 0), ys(B * n * 8, 0), out((B * n + 1) * 8, 0x5A5A5A5A), ws((B + 1) * blk, 0x5A5A5A5A);
    std::vector<uint8_t> st(B + 1, 0x5A);
    const uint32_t x[2][3] = {{1, 2, 4}, {7, 2, 7}}, y[3] = {3, 5, 9};
    for (size_t j = 0; j < B; j++)
      for (size_t s = 0; s < n; s++) {
        xs[(j * n + s) * 8] = x[j][s];
        ys[(j * n + s) * 8] = y[s];
      }
    rc |= dkh_fr_interpolate(n, xs.data(), ys.data(), B, 1, out.data(), ws.data(), st.data());
    rc |= (out[0] == 1 && out[8] == 2 && out[16] == 0 && st[0] == TC_JOB_OK && st[1] == TC_JOB_DUPLICATE_ENTRY && st[2] == 0x5A) ? 0 : 1;
    for (size_t i = n * 8; i < 2 * n * 8; i++) rc |= out[i] == 0 ? 0 : 1;
    for (size_t i = B * blk; i < ws.size(); i++) rc |= ws[i] == 0x5A5A5A5A ? 0 : 1;
    rc |= out[B * n * 8] == 0x5A5A5A5A ? 0 : 1;
  }
  mark("interpolation");
  // sums: 5 g1 twice, 2 g1 .. 8 g1, an identity, a masked term that does not decode; plain and weighted, every lane count and slice count
  {
    const size_t n = 9, B = 1;
    std::vector<uint8_t> pts((n + 1) * 96), w(n * 32), mask(n, 1);
    const uint64_t a[n + 1] = {5, 5, 2, 3, 4, 5, 6, 7, 8, 9}, wt[n] = {3, 3, 0, 1, 9, 11, 1, 2, 64};
    for (size_t k = 0; k <= n; k++) gen_mul(a[k], pts.data() + k * 96);
    for (size_t k = 0; k < n; k++) le32(wt[k], w.data() + k * 32);
    memset(pts.data() + 3 * 96, 0, 96);
    pts[3 * 96] = 0x40;
    memset(pts.data() + 4 * 96, 0x11, 96);
    mask[4] = 0;
    std::vector<uint8_t> out((B + 1) * 96), out1((B + 1) * 96, 0x5A), st(B + 1), bad(n + 1), want(96);
    size_t used[2];
    for (size_t parts : {(size_t)1, (size_t)2, (size_t)8, (size_t)64, (size_t)3}) {
      std::fill(out.begin(), out.end(), (uint8_t)0x5A);
      std::fill(bad.begin(), bad.end(), (uint8_t)0x5A);
      rc |= dkh_g1_sum(0, pts.data(), pts.size(), 96, n, mask.data(), nullptr, B, parts, 1, 1, 1, parts == 1 ? out1.data() : out.data(), st.data(),
                       bad.data(), used);
      if (parts != 1) rc |= memcmp(out.data(), out1.data(), out.size()) ? 1 : 0;
      rc |= (st[0] == TC_JOB_OK && bad[n] == 0x5A && bad[4] == 0) ? 0 : 1;
    }
    gen_mul(5 + 5 + 2 + 5 + 6 + 7 + 8, want.data());
    rc |= memcmp(want.data(), out1.data(), 96) ? 1 : 0;
    const size_t rows = B * n;
    std::vector<uint32_t> rec((n + 1) * kWsumWeightWords);
    std::vector<uint8_t> po((rows + 1) * 96), pst(rows + 1), pok(rows + 1), fo((B + 1) * 96), fs(B + 1);
    gen_mul(5 * 3 + 5 * 3 + 5 * 11 + 6 + 7 * 2 + 8 * 64, want.data());
    for (size_t slices : {(size_t)1, (size_t)2, (size_t)3, n + 3})
      for (size_t parts : {(size_t)1, (size_t)4, (size_t)64}) {
        std::fill(pst.begin(), pst.end(), (uint8_t)0x5A);
        std::fill(pok.begin(), pok.end(), (uint8_t)0x5A);
        rc |= dkh_g1_wsum(0, pts.data(), pts.size(), 96, n, w.data(), n, mask.data(), nullptr, B, parts, slices, 1, nullptr, 1, rows, rec.data(), po.data(),
                          pst.data(), pok.data(), fo.data(), fs.data(), used);
        rc |= used[1] == (slices > n ? n : slices) ? 0 : 1;
        if (used[1] == 1) rc |= (memcmp(want.data(), po.data(), 96) == 0 && pst[0] == TC_JOB_OK && poison(pok.data(), rows + 1)) ? 0 : 1;
        else rc |= (memcmp(want.data(), fo.data(), 96) == 0 && fs[0] == TC_JOB_OK && poison(pst.data(), rows + 1) && pok[0] == 1) ? 0 : 1;
      }
    const uint32_t pick[3] = {8, 0, 5};
    rc |= dkh_g1_wsum(0, pts.data(), pts.size(), 96, n, w.data(), 3, mask.data(), nullptr, B, 2, 2, 1, pick, 1, rows, rec.data(), po.data(), pst.data(),
                      pok.data(), fo.data(), fs.data(), used);
    gen_mul(8 * 64 + 5 * 3 + 5 * 11, want.data());
    rc |= memcmp(want.data(), fo.data(), 96) ? 1 : 0;
  }
  mark("sums");
  // the verdict chain: f(x) = 7 + 3 x, dealers 2 (right), 3 (claims f(3)), 2 again, one rejected
  {
    const size_t P = 4, t_old = 1, deg = 1, stride = 3 * 96;
    std::vector<uint8_t> oc(2 * 96), commits(P * stride);
    gen_mul(7, oc.data());
    gen_mul(3, oc.data() + 96);
    const uint64_t idx[P] = {2, 3, 2, 5};
    const uint8_t accept[P] = {1, 1, 1, 0};
    for (size_t p = 0; p < P; p++)
      for (size_t e = 0; e < 3; e++) gen_mul(e == 0 ? 16 : e + p + 1, commits.data() + p * stride + e * 96);
    std::vector<uint8_t> cs(P + 1, 0x5A), pb(P + 1, 0x5A), du(P + 1, 0x5A), ob(2, 0x5A), ps(P + 1, 0x5A), us(P + 1, 0x5A), wts((P + 1) * 32, 0x5A), st(2, 0x5A);
    std::vector<uint32_t> sp(t_old + 2, 0x5A5A5A5A), ws(5 * (t_old + 1) * 8 + 8, 0x5A5A5A5A);
    std::vector<uint64_t> si(t_old + 2, 0x5A5A5A5A5A5A5A5Aull);
    std::vector<uint8_t> outc((deg + 2) * 96, 0x11), outs(64, 0x11);
    rc |= dkh_reshare_chain(oc.data(), nullptr, t_old, idx, commits.data(), commits.size(), stride, deg, accept, nullptr, nullptr, P, cs.data(), pb.data(),
                            du.data(), ob.data(), ps.data(), us.data(), sp.data(), si.data(), ws.data(), wts.data(), st.data(), outc.data(), outs.data());
    rc |= (cs[0] == TC_JOB_OK && cs[1] == TC_JOB_SHARE_MISMATCH && du[2] == 1 && du[0] == 0 && ps[3] == TC_JOB_OK && ps[2] == TC_JOB_DUPLICATE_ENTRY) ? 0 : 1;
    rc |= (st[0] == TC_JOB_SHARE_MISMATCH && st[1] == 0x5A && us[0] == 0 && us[P] == 0x5A && outc[0] == 0x40 && outc[2 * 96] == 0x11 && outs[0] == 0 &&
           outs[32] == 0x11 && ob[0] == 0 && ob[1] == 0x5A)
              ? 0
              : 1;
  }
  mark("verdict chain");
  printf("dkg_kernels_host: %s\n", rc ? "FAILED" : "ok");
  return rc ? 1 : 0;
}
#endif
