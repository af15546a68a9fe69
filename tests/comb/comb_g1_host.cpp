// TEST HARNESS ONLY (tests/test_comb_g1_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with g++ and exposes
// the two stages of the G1 comb (tc_comb_g1.h) as the kernels of k_comb.hip run them: stage T over one ciphertext's u, stage S
// lane by lane over chunks of `share` holders, and the per-share ladder of the gather form.  Built with -DTC_COMB_G1_COUNT the
// guarded fallback of stage S is counted.  Never linked into libtc_amd.so.  With -DCG_MAIN it is a stand-alone program (for a
// sanitizer build: g++ -fsanitize=address,undefined -DCG_MAIN) that runs every routine once over fixed inputs.
#include "tc_comb_g1.h"
#include "tc_dkg.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
int cg_share() { return kCombG1Share; }
int cg_entries() { return kCombG1Entries; }
// entries96: kCombG1Entries x 96 B, the affine encoding of every entry of the comb of u (column-major, then the two start
// entries); returns 1 when u decoded
int cg_tables(const uint8_t* u96, uint8_t* entries96) {
  std::vector<int32_t> tbl(kCombG1TableWords);
  const bool ok = job_comb_tables_g1(u96, tbl.data());
  for (int i = 0; i < kCombG1Entries; i++) g1_encode_uncompressed(msm_load_entry_g1(tbl.data() + (size_t)i * kMsmEntryWordsG1), entries96 + (size_t)i * 96);
  return ok ? 1 : 0;
}
// out (n x 96 B) / status (n B) = the shares of u by the holders idx[0 .. n) of sk_table (N x 32 B), `share` holders per lane;
// returns the number of holders that took the guarded fallback (-1: not counted in this build)
long cg_decrypt(const uint8_t* sk_table, size_t N, const uint64_t* idx, size_t n, const uint8_t* u96, size_t share, uint8_t* out, uint8_t* status) {
  std::vector<int32_t> tbl(kCombG1TableWords);
  const bool ok = job_comb_tables_g1(u96, tbl.data());
#if defined(TC_COMB_G1_COUNT)
  const unsigned long before = tc_comb_g1_fallbacks;
#endif
  for (size_t s0 = 0; s0 < n; s0 += share) {
    const int cnt = (int)((n - s0 < share) ? n - s0 : share);
    job_comb_decrypt(sk_table, N, idx + s0, cnt, tbl.data(), ok, out + s0 * 96, status ? status + s0 : nullptr);
  }
#if defined(TC_COMB_G1_COUNT)
  return (long)(tc_comb_g1_fallbacks - before);
#else
  return -1;
#endif
}
// the gather form: one ladder per (ciphertext, holder)
void cg_gather(const uint8_t* sk_table, size_t N, const uint64_t* idx, size_t n, const uint8_t* u96, uint8_t* out, uint8_t* status) {
  for (size_t s = 0; s < n; s++) status[s] = job_g1_mul_gather(sk_table, N, idx[s], u96, out + s * 96);
}
// [k] g1, for the harness's own inputs
void cg_g1_mul_gen(uint64_t k, uint8_t* out96) { g1_encode_uncompressed(jac_to_affine(g1_mul_u64(G1Jac::from_affine(g1_generator()), k)), out96); }
}

#if defined(CG_MAIN)
static void le32(uint64_t v, uint8_t* out) {
  memset(out, 0, 32);
  for (int b = 0; b < 8; b++) out[b] = (uint8_t)(v >> (8 * b));
}
int main() {
  int rc = 0;
  const size_t N = 12;
  const uint64_t sk[N] = {0, 1, 2, 3, 4, 5, 77, 0xffffffffffffffffull, 1234567, 9, 10, 11};
  std::vector<uint8_t> table(N * 32), u(96), want(96), ents((size_t)kCombG1Entries * 96);
  for (size_t i = 0; i < N; i++) le32(sk[i], table.data() + i * 32);
  memset(table.data() + 9 * 32, 0xff, 32);                                                    // a scalar >= r
  cg_g1_mul_gen(7, u.data());
  rc |= cg_tables(u.data(), ents.data()) == 1 ? 0 : 1;
  cg_g1_mul_gen(7, want.data());
  rc |= memcmp(ents.data(), want.data(), 96) ? 1 : 0;                                          // entry 0 of column 0 is P
  cg_g1_mul_gen(21, want.data());
  rc |= memcmp(ents.data() + 4 * 96, want.data(), 96) ? 1 : 0;                                 // entry 4 is 3P
  cg_g1_mul_gen(7 * 4 * 3, want.data());
  rc |= memcmp(ents.data() + (8 + 4) * 96, want.data(), 96) ? 1 : 0;                           // column 1: 4 x 3P
  const size_t n = (size_t)kCombG1Share + 3;
  std::vector<uint64_t> idx(n);
  for (size_t s = 0; s < n; s++) idx[s] = (n - 1 - s) % N;                                     // descending, then wrapping
  idx[2] = N;                                                                                  // out of range
  std::vector<uint8_t> out(n * 96), st(n), out2(n * 96), st2(n);
  for (size_t share = 1; share <= (size_t)kCombG1Share; share += kCombG1Share - 1) {
    cg_decrypt(table.data(), N, idx.data(), n, u.data(), share, out.data(), st.data());
    cg_gather(table.data(), N, idx.data(), n, u.data(), out2.data(), st2.data());
    rc |= memcmp(out.data(), out2.data(), n * 96) ? 1 : 0;
    rc |= memcmp(st.data(), st2.data(), n) ? 1 : 0;
    for (size_t s = 0; s < n; s++) {
      const bool bad = idx[s] >= N || idx[s] == 9;
      rc |= (st[s] == (bad ? TC_JOB_INVALID_ENCODING : TC_JOB_OK)) ? 0 : 1;
      if (!bad && sk[idx[s]] < (1ull << 40)) {
        cg_g1_mul_gen(7 * sk[idx[s]], want.data());
        if (sk[idx[s]] == 0) {
          memset(want.data(), 0, 96);
          want[0] = 0x40;
        }
        rc |= memcmp(out.data() + s * 96, want.data(), 96) ? 1 : 0;
      }
    }
  }
  // the identity as u: a valid operand, identity shares; an undecodable u: every output fails
  memset(u.data(), 0, 96);
  u[0] = 0x40;
  rc |= cg_tables(u.data(), ents.data()) == 1 ? 0 : 1;
  cg_decrypt(table.data(), N, idx.data(), 3, u.data(), 8, out.data(), st.data());
  rc |= (st[0] == TC_JOB_OK && st[2] == TC_JOB_INVALID_ENCODING && out[0] == 0x40) ? 0 : 1;
  memset(u.data(), 0x11, 96);
  rc |= cg_tables(u.data(), ents.data()) == 0 ? 0 : 1;
  cg_decrypt(table.data(), N, idx.data(), 3, u.data(), 8, out.data(), st.data());
  rc |= (st[0] == TC_JOB_INVALID_ENCODING && st[1] == TC_JOB_INVALID_ENCODING && out[0] == 0x40 && out[96] == 0x40) ? 0 : 1;
  printf("comb_g1_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
