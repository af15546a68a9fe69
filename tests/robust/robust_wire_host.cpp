// TEST HARNESS ONLY (tests/test_robust_wire_host.py).  Compiles the device headers with g++ and exposes what the wire forms of
// the robust combiners add: the curve-level forms of the three compressed decodes (tc_sqrt.h, MEMBER = false) next to the
// checked ones, and the record-to-source mapping of the selected decode (tc_robust.h selected_source, tc_jobs.h
// job_decompress_selected / job_decompress_selected_g2_x2) run as the kernels of k_mul.hip run it: record by record, pair by
// pair.  Never linked into libtc_amd.so.  With -DRW_MAIN it is a stand-alone program (for a sanitizer build:
// g++ -fsanitize=address,undefined -DRW_MAIN) that runs every routine once over fixed inputs.
#include "tc_jobs.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
// one compressed point; member = 1: the checked decode (job_decompress), 0: the curve-level one.  Returns 1 when it decoded;
// out holds the uncompressed point, or the identity after a failure.
int rw_decode_g1(const uint8_t* in48, int member, uint8_t* out96) {
  return (member ? job_decompress<Fq>(in48, out96) : job_decompress_curve<Fq>(in48, out96)) == TC_JOB_OK;
}
int rw_decode_g2(const uint8_t* in96, int member, uint8_t* out192) {
  return (member ? job_decompress<Fq2>(in96, out192) : job_decompress_curve<Fq2>(in96, out192)) == TC_JOB_OK;
}
// two compressed G2 points through the two-point form; out_b may be null (the odd tail).  ok[0], ok[1].
void rw_decode_g2_x2(const uint8_t* in_a, const uint8_t* in_b, int member, uint8_t* out_a, uint8_t* out_b, uint8_t* ok) {
  G2Affine pa, pb;
  bool oka, okb;
  if (member) g2_decode_compressed_x2<true>(in_a, in_b, pa, pb, oka, okb);
  else g2_decode_compressed_x2<false>(in_a, in_b, pa, pb, oka, okb);
  g2_encode_uncompressed(pa, out_a);
  if (out_b) g2_encode_uncompressed(pb, out_b);
  ok[0] = oka;
  ok[1] = okb;
}

// the source offset of record i, or ~0 for a record without one
uint64_t rw_selected_source(size_t i, size_t N, size_t need, const uint32_t* slot, const uint8_t* enough, size_t cbytes) {
  return (uint64_t)selected_source(i, N, need, slot, enough, cbytes);
}

// The selected decode over jobs x need records, as launch_decompress_selected's kernels walk them.  form: 0 = G1 (one record
// per lane), 1 = G2 (one record per lane pair), 2 = G2 two records per lane pair.  `in` is copied into a buffer of exactly
// jobs * N encodings first, so that a source offset formed from a 0xffffffff slot would lie far outside it.
void rw_decompress_selected(int form, const uint8_t* in, size_t N, size_t need, const uint32_t* slot, const uint8_t* enough, size_t jobs,
                            uint8_t* out, uint8_t* ok) {
  const size_t n = jobs * need, CB = form ? 96 : 48;
  std::vector<uint8_t> src(in, in + jobs * N * CB);
  if (form == 0) {
    for (size_t i = 0; i < n; i++) ok[i] = job_decompress_selected<Fq>(src.data(), N, need, slot, enough, i, out + i * 96);
  } else if (form == 1) {
    for (size_t i = 0; i < n; i++) ok[i] = job_decompress_selected<Fq2>(src.data(), N, need, slot, enough, i, out + i * 192);
  } else {
    for (size_t p = 0; 2 * p < n; p++) {
      const size_t ia = 2 * p;
      const bool has_b = ia + 1 < n;
      const size_t ib = has_b ? ia + 1 : ia;
      bool oka, okb;
      job_decompress_selected_g2_x2(src.data(), N, need, slot, enough, ia, ib, out + ia * 192, has_b ? out + ib * 192 : nullptr, oka, okb);
      ok[ia] = oka;
      if (has_b) ok[ib] = okb;
    }
  }
}
}

#if defined(RW_MAIN)
int main() {
  int rc = 0;
  // the identity, and a malformed encoding: the two inputs that need no curve arithmetic to be told apart
  uint8_t ident1[48] = {0xC0}, ident2[96] = {0xC0}, junk1[48], junk2[96];
  memset(junk1, 0xFF, sizeof junk1);
  memset(junk2, 0xFF, sizeof junk2);
  junk1[0] = junk2[0] = 0x9F;  // compressed, finite, x >= q
  uint8_t o1[96], o2[192], o2b[192], ok2[2];
  for (int member = 0; member < 2; member++) {
    rc |= rw_decode_g1(ident1, member, o1) == 1 && o1[0] == 0x40 ? 0 : 1;
    rc |= rw_decode_g1(junk1, member, o1) == 0 && o1[0] == 0x40 ? 0 : 1;
    rc |= rw_decode_g2(ident2, member, o2) == 1 && o2[0] == 0x40 ? 0 : 1;
    rc |= rw_decode_g2(junk2, member, o2) == 0 && o2[0] == 0x40 ? 0 : 1;
    rw_decode_g2_x2(ident2, junk2, member, o2, o2b, ok2);
    rc |= ok2[0] == 1 && ok2[1] == 0 && o2[0] == 0x40 && o2b[0] == 0x40 ? 0 : 1;
    rw_decode_g2_x2(junk2, junk2, member, o2, nullptr, ok2);
    rc |= ok2[0] == 0 ? 0 : 1;
  }
  // the mapping: B = 3 jobs, N = 10, need = 3, the middle job without enough shares
  const size_t B = 3, N = 10, need = 3;
  uint32_t slot[9] = {0, 4, 9, ~0u, ~0u, ~0u, 1, 2, 3};
  uint8_t enough[3] = {1, 0, 1};
  for (int form = 0; form < 3; form++) {
    const size_t CB = form ? 96 : 48, PB = 2 * CB;
    std::vector<uint8_t> in(B * N * CB, 0);
    for (size_t r = 0; r < B * N; r++) in[r * CB] = 0xC0;  // identities everywhere ...
    in[(0 * N + 4) * CB] = 0x9F;                           // ... but one selected share of job 0, which does not decode
    memset(&in[(0 * N + 4) * CB + 1], 0xFF, CB - 1);
    std::vector<uint8_t> out(B * need * PB, 0xAA), ok(B * need, 0xAA);
    rw_decompress_selected(form, in.data(), N, need, slot, enough, B, out.data(), ok.data());
    for (size_t i = 0; i < B * need; i++) {
      rc |= ok[i] == (i == 1 ? 0 : 1) ? 0 : 1;
      rc |= out[i * PB] == 0x40 ? 0 : 1;
    }
    for (size_t i = 0; i < B * need; i++)
      rc |= rw_selected_source(i, N, need, slot, enough, CB) == (enough[i / need] ? (uint64_t)((i / need) * N + slot[i]) * CB : ~0ull) ? 0 : 1;
  }
  printf("robust_wire_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
