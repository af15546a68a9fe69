// TEST HARNESS ONLY (tests/test_records_host.py).  Compiles tc_records.h -- the segment / chunk / part arithmetic the ragged-sum
// kernels (k_msm.hip k_rec_*) and the host side of tc_verify_g2_records_rlc_batch share -- with g++.  Never linked into
// libtc_amd.so.  With -DRECORDS_MAIN it is a stand-alone program (for a sanitizer build: g++ -fsanitize=address,undefined
// -DRECORDS_MAIN) that walks the same arithmetic over fixed inputs in exactly-sized heap arrays and prints "records_host: ok".
#include "tc_records.h"
#include <stdio.h>
#include <vector>
using namespace tc;

extern "C" {
int rh_chunk() { return kRecChunk; }
uint64_t rh_chunks(uint64_t len) { return rec_chunks(len); }
// first_chunk: J + 1 values written, nothing behind them
uint64_t rh_chunk_ranges(const uint64_t* seg_first, size_t J, uint64_t* first_chunk) { return rec_chunk_ranges(seg_first, J, first_chunk); }
// grp_first: rec_groups(M, group) + 1 values written; returns the number of groups
size_t rh_group_ranges(const uint64_t* rec_off, size_t M, size_t group, uint64_t* grp_first) {
  rec_group_ranges(rec_off, M, group, grp_first);
  return rec_groups(M, group);
}
uint64_t rh_piece_size(uint64_t R, size_t want, size_t most) { return rec_piece_size(R, want, most); }
uint64_t rh_piece_total(const uint64_t* grp_first, size_t NG, uint64_t piece) { return rec_piece_total(grp_first, NG, piece); }
// piece_first: rec_piece_total + 1 values written, grp_piece: NG + 1
void rh_piece_ranges(const uint64_t* grp_first, size_t NG, uint64_t piece, uint64_t* piece_first, uint64_t* grp_piece) {
  rec_piece_ranges(grp_first, NG, piece, piece_first, grp_piece);
}
size_t rh_segment_of_chunk(const uint64_t* first_chunk, size_t J, uint64_t c) { return rec_segment_of_chunk(first_chunk, J, c); }
size_t rh_parts(size_t segments, uint64_t longest, size_t want, size_t most, size_t forced) { return rec_parts(segments, longest, want, most, forced); }
// out: two values (s0, s1)
void rh_part(uint64_t len, size_t g, size_t parts, uint64_t* out) {
  const RecPart p = rec_part(len, g, parts);
  out[0] = p.s0;
  out[1] = p.s1;
}
uint64_t rh_part_trips(uint64_t len, size_t parts) { return rec_part_trips(len, parts); }
}

#if defined(RECORDS_MAIN)
int main() {
  int rc = 0;
  const uint64_t lens[] = {0, 1, 3, 4, 5, 8, 33, 130, 0, 0, 2};
  const size_t M = sizeof(lens) / sizeof(lens[0]);
  std::vector<uint64_t> rec_off(M + 1);
  rec_off[0] = 0;
  for (size_t m = 0; m < M; m++) rec_off[m + 1] = rec_off[m] + lens[m];
  std::vector<uint64_t> fc(M + 1);
  const uint64_t C = rec_chunk_ranges(rec_off.data(), M, fc.data());
  uint64_t want = 0;
  for (size_t m = 0; m < M; m++) {
    rc |= fc[m] == want ? 0 : 1;
    want += (lens[m] + 3) / 4;
  }
  rc |= (C == want && fc[M] == want) ? 0 : 1;
  // every chunk finds its segment, and the segment is never an empty one
  for (uint64_t c = 0; c < C; c++) {
    const size_t j = rec_segment_of_chunk(fc.data(), M, c);
    rc |= (j < M && fc[j] <= c && c < fc[j + 1] && lens[j] != 0) ? 0 : 1;
  }
  for (size_t group : {(size_t)1, (size_t)2, (size_t)3, (size_t)64}) {
    const size_t NG = rec_groups(M, group);
    std::vector<uint64_t> gf(NG + 1), gc(NG + 1);
    rec_group_ranges(rec_off.data(), M, group, gf.data());
    for (size_t g = 0; g <= NG; g++) rc |= gf[g] == rec_off[g * group < M ? g * group : M] ? 0 : 1;
    rc |= gf[NG] == rec_off[M] ? 0 : 1;
    rec_chunk_ranges(gf.data(), NG, gc.data());
    // the pieces of the groups: exactly-sized arrays, every record in exactly one piece, no piece across two groups
    for (uint64_t piece : {(uint64_t)1, (uint64_t)4, (uint64_t)64, (uint64_t)1000}) {
      const uint64_t NP = rec_piece_total(gf.data(), NG, piece);
      std::vector<uint64_t> pf(NP + 1), gp(NG + 1);
      rec_piece_ranges(gf.data(), NG, piece, pf.data(), gp.data());
      rc |= (gp[0] == 0 && gp[NG] == NP && pf[NP] == rec_off[M]) ? 0 : 1;
      for (size_t g = 0; g < NG; g++)
        for (uint64_t q = gp[g]; q < gp[g + 1]; q++)
          rc |= (pf[q] >= gf[g] && pf[q + 1] <= gf[g + 1] && pf[q + 1] > pf[q] && pf[q + 1] - pf[q] <= piece) ? 0 : 1;
    }
  }
  rc |= rec_piece_size(65536, 32768, 32) == 64 ? 0 : 1;
  rc |= rec_piece_size(10, 32768, 32) == 64 ? 0 : 1;
  rc |= rec_piece_size(1 << 20, 32768, 32) == 1024 ? 0 : 1;
  // the parts of a segment tile it, in order, and none is longer than the trip count
  for (uint64_t len : lens)
    for (size_t parts = 1; parts <= 64; parts *= 2) {
      uint64_t at = 0;
      for (size_t g = 0; g < parts; g++) {
        const RecPart p = rec_part(len, g, parts);
        rc |= (p.s0 == at && p.s1 >= p.s0 && p.s1 - p.s0 <= rec_part_trips(len, parts)) ? 0 : 1;
        at = p.s1;
      }
      rc |= at == len ? 0 : 1;
    }
  rc |= rec_parts(1, 130, 65536, 32) == 32 ? 0 : 1;
  rc |= rec_parts(1 << 20, 130, 65536, 32) == 1 ? 0 : 1;
  rc |= rec_parts(7, 3, 65536, 64) == 1 ? 0 : 1;
  rc |= rec_parts(7, 4, 65536, 64) == 2 ? 0 : 1;
  rc |= rec_parts(7, 4, 65536, 64, 16) == 16 ? 0 : 1;
  printf("records_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
