// TEST HARNESS ONLY (tests/test_dkg_reshare_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with g++ and
// exposes the routines of the DKG resharing (tc_dkg.h): the weighted G1 sum of one output as the lanes of k_g1_wsum run it -- the
// weights recoded once per term, the partial sums of lanes g = 0 .. parts-1 one after the other, then the kernel's xor tree of
// complete additions --, the weighted Fr sum, the selection helper and the constant check.  Never linked into libtc_amd.so.  With
// -DDR_MAIN it is a stand-alone program (for a sanitizer build: g++ -fsanitize=address,undefined -DDR_MAIN) that runs every
// routine once over fixed inputs.
#include "tc_dkg.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
// out = sum_{k < n, included} w[k] pts[k * term_stride] with `parts` lanes; w: n x 32 B LE; member / term_bad as in dg_g1_sum
int dr_g1_wsum(const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* w, const uint8_t* mask, const uint8_t* member, size_t parts,
               uint8_t* out96, uint8_t* term_bad) {
  std::vector<uint32_t> rec(n * kWsumWeightWords + 1);
  for (size_t k = 0; k < n; k++) wsum_recode_weight(w + k * 32, rec.data() + k * kWsumWeightWords);
  std::vector<G1Jac> r(parts);
  std::vector<int> good(parts);
  for (size_t g = 0; g < parts; g++) {
    bool ok;
    r[g] = job_g1_wsum_part(pts, term_stride, rec.data(), mask, member, 1, sum_part(n, g, parts), ok, term_bad);
    good[g] = ok ? 1 : 0;
  }
  for (size_t d = 1; d < parts; d <<= 1) {  // every lane adds its partner's value of the round before
    std::vector<G1Jac> nr(parts);
    std::vector<int> ng(parts);
    for (size_t g = 0; g < parts; g++) {
      nr[g] = jac_add(r[g], r[g ^ d]);
      ng[g] = good[g] & good[g ^ d];
    }
    r = nr;
    good = ng;
  }
  g1_encode_uncompressed(good[0] ? jac_to_affine(r[0]) : G1Affine::infinity(), out96);
  return good[0] ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
// the same over the terms sel[0 .. n_sel) only (the selected dealers of a resharing): the lanes split the positions of sel
int dr_g1_wsum_sel(const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* w, const uint8_t* mask, const uint32_t* sel, size_t n_sel,
                   size_t parts, uint8_t* out96) {
  std::vector<uint32_t> rec(n * kWsumWeightWords + 1);
  for (size_t k = 0; k < n; k++) wsum_recode_weight(w + k * 32, rec.data() + k * kWsumWeightWords);
  std::vector<G1Jac> r(parts);
  bool good = true;
  for (size_t g = 0; g < parts; g++) {
    bool ok;
    r[g] = job_g1_wsum_part(pts, term_stride, rec.data(), mask, nullptr, 1, sum_part(n_sel, g, parts), ok, nullptr, sel);
    good = good && ok;
  }
  for (size_t d = 1; d < parts; d <<= 1) {
    std::vector<G1Jac> nr(parts);
    for (size_t g = 0; g < parts; g++) nr[g] = jac_add(r[g], r[g ^ d]);
    r = nr;
  }
  g1_encode_uncompressed(good ? jac_to_affine(r[0]) : G1Affine::infinity(), out96);
  return good ? TC_JOB_OK : TC_JOB_INVALID_ENCODING;
}
void dr_slice_part(size_t n, size_t s, size_t slices, size_t g, size_t parts, size_t* out2) {
  const SumPart p = wsum_slice_part(n, s, slices, g, parts);
  out2[0] = p.k0;
  out2[1] = p.k1;
}
int dr_fr_wsum(const uint8_t* vals, size_t term_stride, size_t n, const uint8_t* w, const uint8_t* mask, uint8_t* out32) {
  return job_fr_wsum(vals, term_stride, n, w, mask, out32);
}
// used, dup: P bytes; sel_part / sel_idx: t_old + 1 entries; returns 1 when enough parts are accepted
int dr_select(const uint8_t* accept, const uint64_t* dealer_idx, size_t t_old, size_t P, uint8_t* used, uint32_t* sel_part, uint64_t* sel_idx,
              uint8_t* dup) {
  return reshare_select(accept, dealer_idx, t_old, P, used, sel_part, sel_idx, dup) ? 1 : 0;
}
// lambda_i at zero of the abscissae idx[i] + 1 (out: (t + 1) x 32 B LE)
int dr_lagrange(const uint64_t* idx, size_t t, uint8_t* out) {
  std::vector<uint32_t> lam((t + 1) * 8), ws(4 * (t + 1) * 8);
  const uint8_t st = lagrange_all_at_zero(idx, (int)t, lam.data(), ws.data());
  for (size_t i = 0; i < (t + 1) * 8; i++)
    for (int b = 0; b < 4; b++) out[i * 4 + b] = (uint8_t)(lam[i] >> (8 * b));
  return st;
}
int dr_constant_check(const uint8_t* old_commit, size_t t_old, uint64_t idx, const uint8_t* c0) {
  return job_reshare_constant_check(old_commit, t_old, idx, c0);
}
// [k] g1, for the harness's own inputs
void dr_g1_mul_gen(uint64_t k, uint8_t* out96) { g1_encode_uncompressed(jac_to_affine(g1_mul_u64(G1Jac::from_affine(g1_generator()), k)), out96); }
}

#if defined(DR_MAIN)
static void le32(uint64_t v, uint8_t* out) {
  memset(out, 0, 32);
  for (int b = 0; b < 8; b++) out[b] = (uint8_t)(v >> (8 * b));
}
int main() {
  const size_t n = 9;
  std::vector<uint8_t> pts(n * 96), w(n * 32), out(96), out1(96), want(96), vals(n * 32), mask(n, 1), bad(n, 0);
  const uint64_t a[n] = {5, 5, 2, 3, 4, 5, 6, 7, 8}, ws[n] = {3, 3, 0, 1, 9, 11, 1, 2, 64};
  uint64_t sum = 0;
  for (size_t k = 0; k < n; k++) {
    dr_g1_mul_gen(a[k], pts.data() + k * 96);
    le32(ws[k], w.data() + k * 32);
    if (k != 3 && k != 4) sum += a[k] * ws[k];
  }
  memset(pts.data() + 3 * 96, 0, 96);
  pts[3 * 96] = 0x40;                                                                      // an identity in the middle
  memset(pts.data() + 4 * 96, 0x11, 96);                                                   // garbage, masked out
  mask[4] = 0;
  int rc = 0;
  for (size_t parts = 1; parts <= 64; parts *= 2) {
    rc |= dr_g1_wsum(pts.data(), 96, n, w.data(), mask.data(), nullptr, parts, parts == 1 ? out1.data() : out.data(), bad.data());
    if (parts > 1) rc |= memcmp(out.data(), out1.data(), 96) ? 1 : 0;
  }
  dr_g1_mul_gen(sum, want.data());
  rc |= memcmp(want.data(), out1.data(), 96) ? 1 : 0;
  mask[4] = 1;
  rc |= dr_g1_wsum(pts.data(), 96, n, w.data(), mask.data(), nullptr, 4, out.data(), bad.data()) == TC_JOB_INVALID_ENCODING ? 0 : 1;
  rc |= (bad[4] == 1 && out[0] == 0x40) ? 0 : 1;
  mask[4] = 0;
  memset(w.data() + 7 * 32, 0xff, 32);                                                     // a weight >= r
  rc |= dr_g1_wsum(pts.data(), 96, n, w.data(), mask.data(), nullptr, 2, out.data(), nullptr) == TC_JOB_INVALID_ENCODING ? 0 : 1;
  rc |= dr_g1_wsum(pts.data(), 96, 0, w.data(), nullptr, nullptr, 8, out.data(), nullptr);
  size_t sp2[2], next = 0;
  for (size_t s = 0; s < 3; s++)
    for (size_t g = 0; g < 4; g++) {                                                       // 3 slices x 4 lanes tile 0 .. n
      dr_slice_part(n, s, 3, g, 4, sp2);
      rc |= (sp2[0] == next && sp2[1] >= sp2[0]) ? 0 : 1;
      next = sp2[1];
    }
  rc |= next == n ? 0 : 1;
  const uint32_t pick[3] = {8, 0, 5};                                                      // three of the nine terms, by number
  rc |= dr_g1_wsum_sel(pts.data(), 96, n, w.data(), mask.data(), pick, 3, 4, out.data());
  dr_g1_mul_gen(a[8] * ws[8] + a[0] * ws[0] + a[5] * ws[5], want.data());
  rc |= memcmp(want.data(), out.data(), 96) ? 1 : 0;
  for (size_t i = 0; i < vals.size(); i++) vals[i] = (i % 32 == 31) ? 0 : (uint8_t)(i * 101 + 3);
  le32(2, w.data() + 7 * 32);
  rc |= dr_fr_wsum(vals.data(), 32, n, w.data(), mask.data(), out.data());
  rc |= dr_fr_wsum(vals.data(), 32, 0, w.data(), nullptr, out.data());
  // selection: six parts, one rejected, one repeated index, index 2^64 - 1; guard bytes behind every output
  const uint8_t accept[6] = {1, 0, 1, 1, 1, 1};
  const uint64_t idx[6] = {4, 9, ~0ull, 4, 0, 7};
  uint8_t used[7], dup[7];
  uint32_t sp[4];
  uint64_t si[4];
  used[6] = dup[6] = 0xA5;
  sp[3] = 0xA5A5A5A5u;
  si[3] = 0xA5A5A5A5A5A5A5A5ull;
  rc |= dr_select(accept, idx, 2, 6, used, sp, si, dup) == 1 ? 0 : 1;
  rc |= (used[0] && !used[1] && used[2] && used[3] && !used[4] && !used[5] && dup[3] == 1 && dup[0] + dup[1] + dup[2] + dup[4] + dup[5] == 0) ? 0 : 1;
  rc |= (sp[0] == 0 && sp[1] == 2 && sp[2] == 3 && si[1] == ~0ull) ? 0 : 1;
  rc |= (used[6] == 0xA5 && dup[6] == 0xA5 && sp[3] == 0xA5A5A5A5u && si[3] == 0xA5A5A5A5A5A5A5A5ull) ? 0 : 1;
  rc |= dr_select(accept, idx, 5, 6, used, sp, si, dup) == 0 ? 0 : 1;
  rc |= dr_select(nullptr, idx, 0, 0, used, sp, si, dup) == 0 ? 0 : 1;
  // Lagrange weights of {1, 2^64, 8} and the constant check of old node 2 under f(x) = 7 + 3 x: f(3) = 16
  const uint64_t li[3] = {0, ~0ull, 7};
  std::vector<uint8_t> lam(3 * 32), oc(2 * 96), c0(96);
  rc |= dr_lagrange(li, 2, lam.data());
  dr_g1_mul_gen(7, oc.data());
  dr_g1_mul_gen(3, oc.data() + 96);
  dr_g1_mul_gen(16, c0.data());
  rc |= dr_constant_check(oc.data(), 1, 2, c0.data()) == TC_JOB_OK ? 0 : 1;
  rc |= dr_constant_check(oc.data(), 1, 3, c0.data()) == TC_JOB_SHARE_MISMATCH ? 0 : 1;
  rc |= dr_constant_check(oc.data(), 1, ~0ull, c0.data()) == TC_JOB_SHARE_MISMATCH ? 0 : 1;
  rc |= dr_constant_check(oc.data(), 1, 2, pts.data() + 4 * 96) == TC_JOB_INVALID_ENCODING ? 0 : 1;
  printf("dkg_reshare_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
