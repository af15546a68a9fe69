// Host leg of the blame-by-bisection kernels (tests/test_blame_dev_host.py): the header routines k_blame.hip calls --
// blame_call_seed, job_blame_leaf<F> (the short-scalar leaf multiplications in G1 and G2) and job_blame_range_part<F> -- run by
// g++ with -DTC_BOUND_CHECK over the kernels' buffers: the leaves one after the other, the parts of a range one after the other,
// then the kernel's xor tree of jac_add and its one conversion to affine (the pattern of tests/device/manypoint_host.cpp).  What
// it cannot see is the kernels' own text (lane pairs, the shuffle merge, the indexing): that is the GPU suite.
// With -DBD_MAIN it is a stand-alone program over a fixed short case list (for a g++ -fsanitize=address,undefined build).
// Test code only: never linked into libtc_amd.so.
#include "../../threshold_crypto_amd/csrc/tc_blame_jobs.h"

#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tc;

namespace {
void key_words(const uint8_t* b, uint32_t* w) {
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
template <class F>
void leaves(const uint8_t* seed32, uint64_t leaf0, const uint8_t* pts, size_t period, uint8_t* live, size_t n, int32_t* out) {
  uint32_t key[8];
  key_words(seed32, key);
  for (size_t r = 0; r < n; r++)
    job_blame_leaf<F>(key, leaf0 + r, pts + (period ? r % period : r) * PointIO<F>::BYTES, live ? live + r : nullptr, true, out + r * BlameLeaf<F>::WORDS);
}
template <class F>
void range_sum(const int32_t* lv, size_t lo, size_t hi, size_t parts, uint8_t* out) {
  std::vector<Jac<F>> r(parts);
  for (size_t g = 0; g < parts; g++) r[g] = job_blame_range_part<F>(lv, lo, hi, g, parts);
  for (size_t d = 1; d < parts; d <<= 1) {  // every lane (pair) adds its partner's value of the round before
    std::vector<Jac<F>> nr(parts);
    for (size_t g = 0; g < parts; g++) nr[g] = jac_add(r[g], r[g ^ d]);
    r = nr;
  }
  PointIO<F>::encode(jac_to_affine(r[0]), out);
}
}  // namespace

extern "C" {
size_t bdh_leaf_bytes(int g2) { return (size_t)(g2 ? kBlameLeafWordsG2 : kBlameLeafWordsG1) * 4; }
void bdh_call_seed(const uint8_t* key32, uint64_t call, uint8_t* seed32) {
  uint32_t key[8], seed[8];
  key_words(key32, key);
  blame_call_seed(key, call, seed);
  for (int w = 0; w < 8; w++)
    for (int b = 0; b < 4; b++) seed32[4 * w + b] = (uint8_t)(seed[w] >> (8 * b));
}
void bdh_digits(const uint8_t* seed32, uint64_t leaf, uint64_t* d4) {
  uint32_t key[8];
  key_words(seed32, key);
  blame_digits(key, leaf, d4);
}
void bdh_leaves(int g2, const uint8_t* seed32, uint64_t leaf0, const uint8_t* pts, size_t period, uint8_t* live, size_t n, int32_t* out) {
  if (g2) leaves<Fq2>(seed32, leaf0, pts, period, live, n, out);
  else leaves<Fq>(seed32, leaf0, pts, period, live, n, out);
}
void bdh_range_sum(int g2, const int32_t* lv, size_t lo, size_t hi, size_t parts, uint8_t* out) {
  if (g2) range_sum<Fq2>(lv, lo, hi, parts, out);
  else range_sum<Fq>(lv, lo, hi, parts, out);
}
}

#if defined(BD_MAIN)
#include "../../threshold_crypto_amd/csrc/tc_dkg.h"  // g1_mul_u64, for the inputs
int main() {
  int rc = 0;
  const size_t n = 5;
  uint8_t seed[32], key[32];
  for (int i = 0; i < 32; i++) key[i] = (uint8_t)(3 * i + 1);
  bdh_call_seed(key, 7, seed);
  // G1: [i + 2] g1, slot 1 the identity's encoding, slot 3 not live
  std::vector<uint8_t> p1(n * 96), live(n, 1), o1(96), o2(96), o4(96);
  for (size_t i = 0; i < n; i++) g1_encode_uncompressed(jac_to_affine(g1_mul_u64(G1Jac::from_affine(g1_generator()), i + 2)), p1.data() + i * 96);
  memset(p1.data() + 96, 0, 96);
  p1[96] = 0x40;
  live[3] = 0;
  std::vector<int32_t> l1(n * kBlameLeafWordsG1);
  bdh_leaves(0, seed, 10, p1.data(), 0, live.data(), n, l1.data());
  for (size_t parts = 1; parts <= 4; parts *= 2) {
    bdh_range_sum(0, l1.data(), 0, n, parts, parts == 1 ? o1.data() : o2.data());
    if (parts > 1) rc |= memcmp(o1.data(), o2.data(), 96) ? 1 : 0;
  }
  bdh_range_sum(0, l1.data(), 1, 2, 1, o4.data());  // the identity's leaf
  rc |= o4[0] == 0x40 ? 0 : 1;
  bdh_range_sum(0, l1.data(), 3, 4, 2, o4.data());  // a slot that is not live
  rc |= o4[0] == 0x40 ? 0 : 1;
  rc |= o1[0] == 0x40 ? 1 : 0;
  // G2: the generator in every slot; slot 2 undecodable (clears its live byte)
  std::vector<uint8_t> p2(n * 192), live2(n, 1), q1(192), q2(192);
  for (size_t i = 0; i < n; i++)
    g2_encode_uncompressed(G2Affine{Fq2::make(Fq::from_mont384(G2_GEN_X0), Fq::from_mont384(G2_GEN_X1)),
                                    Fq2::make(Fq::from_mont384(G2_GEN_Y0), Fq::from_mont384(G2_GEN_Y1)), false},
                           p2.data() + i * 192);
  p2[2 * 192] = 0x1f;
  memset(p2.data() + 2 * 192 + 1, 0xff, 191);
  std::vector<int32_t> l2(n * kBlameLeafWordsG2);
  bdh_leaves(1, seed, 10, p2.data(), 0, live2.data(), n, l2.data());
  rc |= (live2[2] == 0 && live2[0] == 1 && live2[4] == 1) ? 0 : 1;
  for (size_t parts = 1; parts <= 2; parts *= 2) {
    bdh_range_sum(1, l2.data(), 0, n, parts, parts == 1 ? q1.data() : q2.data());
    if (parts > 1) rc |= memcmp(q1.data(), q2.data(), 192) ? 1 : 0;
  }
  bdh_range_sum(1, l2.data(), 2, 3, 1, q2.data());
  rc |= q2[0] == 0x40 ? 0 : 1;
  // a range longer than a wave at a wave's worth of parts: 70 G1 leaves of one row of 5 points (the key-share form), slots 3 .. 69
  {
    const size_t m = 70;
    std::vector<int32_t> l3(m * kBlameLeafWordsG1);
    std::vector<uint8_t> r1(96), r64(96), r3(96);
    bdh_leaves(0, seed, 0, p1.data(), n, nullptr, m, l3.data());
    bdh_range_sum(0, l3.data(), 3, m, 1, r1.data());
    bdh_range_sum(0, l3.data(), 3, m, 64, r64.data());
    bdh_range_sum(0, l3.data(), 3, m, 32, r3.data());
    rc |= (memcmp(r1.data(), r64.data(), 96) || memcmp(r1.data(), r3.data(), 96) || r1[0] == 0x40) ? 1 : 0;
    bdh_range_sum(0, l3.data(), 66, 67, 64, r3.data());  // leaf 66 is point 1, the identity's encoding: 63 parts without a term beside it
    rc |= r3[0] == 0x40 ? 0 : 1;
  }
  printf("blame_dev_host: %s\n", rc ? "FAILED" : "ok");
  return rc ? 1 : 0;
}
#endif
