// TEST HARNESS ONLY (tests/test_dkg_generate_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with g++ and
// exposes the routines of the DKG finalisation (tc_dkg.h): sum_part, the G1 sum of one output as the lanes of k_g1_sum run it
// -- the partial sums of lanes g = 0 .. parts-1 one after the other, then the kernel's xor tree of complete additions --, the
// Fr sum and the interpolation at zero.  Never linked into libtc_amd.so.  With -DDG_MAIN it is a stand-alone program (for a
// sanitizer build: g++ -fsanitize=address,undefined -DDG_MAIN) that runs every routine once over fixed inputs.
#include "tc_dkg.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
void dg_sum_part(size_t n, size_t g, size_t parts, size_t* out2) {
  const SumPart p = sum_part(n, g, parts);
  out2[0] = p.k0;
  out2[1] = p.k1;
}
// out = sum_{k < n, included} pts[k * term_stride] with `parts` lanes; member: n bytes or null (the verdicts of a membership
// test); term_bad: n zeroed bytes or null.  Returns the job status.
int dg_g1_sum(const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* mask, const uint8_t* member, size_t parts, uint8_t* out96,
              uint8_t* term_bad) {
  std::vector<G1Jac> r(parts);
  std::vector<int> good(parts);
  for (size_t g = 0; g < parts; g++) {
    bool ok;
    r[g] = job_g1_sum_part(pts, term_stride, mask, member, 1, sum_part(n, g, parts), ok, term_bad);
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
int dg_fr_sum(const uint8_t* vals, size_t term_stride, size_t n, const uint8_t* mask, uint8_t* out32) {
  return job_fr_sum(vals, term_stride, n, mask, out32);
}
int dg_fr_interpolate_at_zero(size_t n, const uint64_t* xs, const uint8_t* vals, uint8_t* out32) {
  return job_fr_interpolate_at_zero(n, xs, vals, out32);
}
// [k] g1, for the harness's own inputs
void dg_g1_mul_gen(uint64_t k, uint8_t* out96) { g1_encode_uncompressed(jac_to_affine(g1_mul_u64(G1Jac::from_affine(g1_generator()), k)), out96); }
}

#if defined(DG_MAIN)
int main() {
  const size_t n = 9;
  std::vector<uint8_t> pts(n * 96), out(96), out1(96), vals(n * 32), mask(n, 1), bad(n, 0);
  for (size_t k = 0; k < n; k++) dg_g1_mul_gen(k < 2 ? 5 : k, pts.data() + k * 96);       // 5 g1 twice, 2 g1 .. 8 g1
  memset(pts.data() + 3 * 96, 0, 96);
  pts[3 * 96] = 0x40;                                                                      // an identity in the middle
  memset(pts.data() + 4 * 96, 0x11, 96);                                                   // garbage, masked out
  mask[4] = 0;
  int rc = 0;
  for (size_t parts = 1; parts <= 64; parts *= 2) {
    rc |= dg_g1_sum(pts.data(), 96, n, mask.data(), nullptr, parts, parts == 1 ? out1.data() : out.data(), bad.data());
    if (parts > 1) rc |= memcmp(out.data(), out1.data(), 96) ? 1 : 0;
  }
  dg_g1_mul_gen(5 + 5 + 2 + 5 + 6 + 7 + 8, out.data());
  rc |= memcmp(out.data(), out1.data(), 96) ? 1 : 0;
  mask[4] = 1;
  rc |= dg_g1_sum(pts.data(), 96, n, mask.data(), nullptr, 4, out.data(), bad.data()) == TC_JOB_INVALID_ENCODING ? 0 : 1;
  rc |= (bad[4] == 1 && out[0] == 0x40) ? 0 : 1;
  rc |= dg_g1_sum(pts.data(), 96, 0, nullptr, nullptr, 8, out.data(), nullptr);
  for (size_t i = 0; i < vals.size(); i++) vals[i] = (i % 32 == 31) ? 0 : (uint8_t)(i * 101 + 3);
  rc |= dg_fr_sum(vals.data(), 32, n, mask.data(), out.data());
  rc |= dg_fr_sum(vals.data(), 32, 0, nullptr, out.data());
  const uint64_t xs[n] = {0, 1, 2, 4, 5, 7, 9, 11, ~0ull};
  rc |= dg_fr_interpolate_at_zero(n, xs, vals.data(), out.data());
  rc |= memcmp(out.data(), vals.data(), 32) ? 1 : 0;                                        // the sample at abscissa 0
  rc |= dg_fr_interpolate_at_zero(0, xs, vals.data(), out.data());
  const uint64_t dup[3] = {3, 8, 3};
  rc |= dg_fr_interpolate_at_zero(3, dup, vals.data(), out.data()) == TC_JOB_DUPLICATE_ENTRY ? 0 : 1;
  size_t part[2];
  for (size_t g = 0, next = 0; g < 64; g++) {
    dg_sum_part(n, g, 64, part);
    rc |= (part[0] == next && part[1] >= part[0]) ? 0 : 1;
    next = part[1];
    if (g == 63) rc |= next == n ? 0 : 1;
  }
  printf("dkg_generate_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
