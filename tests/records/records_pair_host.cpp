// TEST HARNESS ONLY (tests/test_records_pair_host.py).  Compiles the PAIRED part of tc_records.h -- where a lane of
// k_rec_tables_g1_pair / k_rec_ladder_g1_pair (k_msm.hip) finds its work, and where the leader lane of a sum writes -- with g++.
// Never linked into libtc_amd.so.  With -DRECORDS_PAIR_MAIN it is a stand-alone program (for a sanitizer build: g++
// -fsanitize=address,undefined -DRECORDS_PAIR_MAIN) that walks the same arithmetic over fixed inputs in exactly-sized heap arrays
// and prints "records_pair_host: ok".
#include "tc_records.h"
#include <stdio.h>
#include <vector>
using namespace tc;

extern "C" {
uint64_t rp_point_bytes() { return kRecPairPoint; }
uint64_t rp_tables_lanes(uint64_t chunks) { return rec_pair_tables_lanes(chunks); }
uint64_t rp_ladder_lanes(size_t J, size_t parts) { return rec_pair_ladder_lanes(J, parts); }
uint64_t rp_out(size_t j, size_t half) { return rec_pair_out(j, half); }
// stage T: out = 4 values per lane t < 2 first_chunk[J]: (half, chunk in its half, segment, first table place of the chunk)
void rp_tables_map(const uint64_t* first_chunk, size_t J, uint64_t* out) {
  const uint64_t chunks = first_chunk[J], lanes = rec_pair_tables_lanes(chunks);
  for (uint64_t t = 0; t < lanes; t++) {
    const RecPairChunk h = rec_pair_chunk(t, chunks);
    const size_t j = rec_segment_of_chunk(first_chunk, J, h.c);
    out[4 * t] = h.half;
    out[4 * t + 1] = h.c;
    out[4 * t + 2] = j;
    out[4 * t + 3] = rec_pair_place(h.half, first_chunk[j], chunks) + (h.c - first_chunk[j]) * kRecChunk;
  }
}
// stage L: out = 4 values per lane < 2 J parts: (segment, half, part, byte offset of the sum's result)
void rp_ladder_map(size_t J, size_t parts, uint64_t* out) {
  const size_t lanes = rec_pair_ladder_lanes(J, parts);
  for (size_t l = 0; l < lanes; l++) {
    const RecPairLane w = rec_pair_lane(l, parts);
    out[4 * l] = w.j;
    out[4 * l + 1] = w.half;
    out[4 * l + 2] = w.g;
    out[4 * l + 3] = rec_pair_out(w.j, w.half);
  }
}
}

#if defined(RECORDS_PAIR_MAIN)
int main() {
  int rc = 0;
  const uint64_t lens[] = {130, 0, 1, 3, 4, 5, 33, 0, 0, 2};
  const size_t J = sizeof(lens) / sizeof(lens[0]);
  std::vector<uint64_t> seg(J + 1), fc(J + 1);
  seg[0] = 0;
  for (size_t j = 0; j < J; j++) seg[j + 1] = seg[j] + lens[j];
  const uint64_t C = rec_chunk_ranges(seg.data(), J, fc.data());
  // stage T: every table place of both halves is owned by exactly one lane, half 1 behind half 0
  std::vector<uint64_t> map(4 * rec_pair_tables_lanes(C));
  rp_tables_map(fc.data(), J, map.data());
  std::vector<int> owner(2 * C * kRecChunk, 0);
  for (uint64_t t = 0; t < 2 * C; t++) {
    const uint64_t half = map[4 * t], c = map[4 * t + 1], j = map[4 * t + 2], place = map[4 * t + 3];
    rc |= (half == (t >= C ? 1u : 0u) && c == t - half * C && j < J && lens[j] != 0 && fc[j] <= c && c < fc[j + 1]) ? 0 : 1;
    rc |= place == (half * C + c) * kRecChunk ? 0 : 1;
    for (int k = 0; k < kRecChunk && place + k < owner.size(); k++) owner[place + k]++;
  }
  for (int n : owner) rc |= n == 1 ? 0 : 1;
  // stage L: every (segment, half, part) once, a sum's lanes adjacent and inside one wave, the twin sums next to each other
  for (size_t parts = 1; parts <= 64; parts *= 2) {
    const size_t lanes = rec_pair_ladder_lanes(J, parts);
    std::vector<uint64_t> lm(4 * lanes);
    rp_ladder_map(J, parts, lm.data());
    std::vector<int> seen(2 * J * parts, 0);
    for (size_t l = 0; l < lanes; l++) {
      const uint64_t j = lm[4 * l], half = lm[4 * l + 1], g = lm[4 * l + 2], off = lm[4 * l + 3];
      rc |= (j < J && half < 2 && g < parts) ? 0 : 1;
      if (j < J && half < 2 && g < parts) seen[(2 * j + half) * parts + g]++;
      rc |= l == (2 * j + half) * parts + g ? 0 : 1;
      rc |= (l - g) / 64 == (l - g + parts - 1) / 64 ? 0 : 1;  // the lanes of one sum: one wave
      rc |= off == (2 * j + half) * 96 ? 0 : 1;
    }
    for (int n : seen) rc |= n == 1 ? 0 : 1;
    // the lanes behind the last segment of the last wave name no segment
    for (size_t l = lanes; l < (lanes + 63) / 64 * 64; l++) rc |= rec_pair_lane(l, parts).j >= J ? 0 : 1;
  }
  printf("records_pair_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
