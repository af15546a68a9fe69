// Ragged sums for tc_verify_g2_records_rlc_batch / tc_verify_sig_records_rlc_batch (k_msm.hip k_rec_*): the
// arithmetic that maps SEGMENTS of a record array -- the records of one message, or of one group of messages -- to the places
// of the two-stage kernels.  A segment of `len` records owns rec_chunks(len) chunks of kRecChunk places; the places behind its
// last record are identity places (stage T pads them, stage L never visits them), so a chunk never straddles two segments
// and an operand that does not decode fails exactly one segment.  Segment j's tables and digit codes sit where a job of
// launch_msm_g2 / launch_msm_g1 with n = len would keep them, only at first_chunk[j] instead of j * chunks.
// Plain host+device code: the kernels, the host side of the entry (tc_api.hip) and tests/records/records_host.cpp (g++) share it.
#pragma once
#include "tc_common.h"

namespace tc {

constexpr int kRecChunk = 4;  // = kMsmChunk (k_msm.hip asserts it)

TC_HD uint64_t rec_chunks(uint64_t len) { return (len + kRecChunk - 1) / kRecChunk; }

// first_chunk[j] (j <= J) = the chunks of the segments before j, seg_first[j] .. seg_first[j + 1] being segment j's records
// (J + 1 non-decreasing values).  Returns first_chunk[J], the chunks of the launch.
TC_HD uint64_t rec_chunk_ranges(const uint64_t* seg_first, size_t J, uint64_t* first_chunk) {
  uint64_t c = 0;
  for (size_t j = 0; j < J; j++) {
    first_chunk[j] = c;
    c += rec_chunks(seg_first[j + 1] - seg_first[j]);
  }
  first_chunk[J] = c;
  return c;
}

// groups of `group` >= 1 consecutive messages, the last one possibly short
TC_HD size_t rec_groups(size_t M, size_t group) { return (M + group - 1) / group; }
// grp_first[g] (g <= rec_groups(M, group)) = the first record of group g: a group's records are contiguous
TC_HD void rec_group_ranges(const uint64_t* rec_off, size_t M, size_t group, uint64_t* grp_first) {
  const size_t NG = rec_groups(M, group);
  for (size_t g = 0; g <= NG; g++) {
    const size_t m = g * group < M ? g * group : M;
    grp_first[g] = rec_off[m];
  }
}

// The G2 sum of a group runs in two levels when the group is long: its records are cut into PIECES of at most `piece` records
// (a piece never straddles two groups; pieces follow each other like the records do), every piece is a segment of the first
// launch, and the sums of a group's pieces are the records of a second, small launch with unit scalars.  One wave (`most` lane
// pairs) works on a piece, so pieces of rec_piece_size records give a launch of R records `want` lane pairs with at least two
// records each -- never fewer than 2 * most records per piece.
TC_HD uint64_t rec_piece_size(uint64_t R, size_t want, size_t most) {
  const uint64_t waves = want / most ? want / most : 1;
  const uint64_t piece = (R + waves - 1) / waves;
  return piece < 2 * (uint64_t)most ? 2 * (uint64_t)most : piece;
}
// pieces of all groups: sum_g ceil(len_g / piece)
TC_HD uint64_t rec_piece_total(const uint64_t* grp_first, size_t NG, uint64_t piece) {
  uint64_t n = 0;
  for (size_t g = 0; g < NG; g++) n += (grp_first[g + 1] - grp_first[g] + piece - 1) / piece;
  return n;
}
// piece_first[p] (p <= rec_piece_total) = the first record of piece p; grp_piece[g] (g <= NG) = the first piece of group g
TC_HD void rec_piece_ranges(const uint64_t* grp_first, size_t NG, uint64_t piece, uint64_t* piece_first, uint64_t* grp_piece) {
  uint64_t p = 0;
  for (size_t g = 0; g < NG; g++) {
    grp_piece[g] = p;
    for (uint64_t r = grp_first[g]; r < grp_first[g + 1]; r += piece) piece_first[p++] = r;
  }
  grp_piece[NG] = p;
  piece_first[p] = grp_first[NG];
}

// the segment that owns chunk c < first_chunk[J]: the one j with first_chunk[j] <= c < first_chunk[j + 1] (segments without
// records own no chunk and are never the answer)
TC_HD size_t rec_segment_of_chunk(const uint64_t* first_chunk, size_t J, uint64_t c) {
  size_t lo = 0, hi = J;  // first_chunk[lo] <= c < first_chunk[hi]
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (first_chunk[mid] <= c) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Stage L splits every segment of a launch over `parts` lanes (G1) / lane pairs (G2), a power of two of at most `most` (a
// wave's worth), so a segment never spans two waves: the smallest that gives the launch `want` lanes / lane pairs (one wave per
// SIMD), with at least two records per part in the LONGEST segment.  forced (tests, the probe: TC_RECORDS_PARTS): that many
// when it is a power of two within `most`.
TC_HD size_t rec_parts(size_t segments, uint64_t longest, size_t want, size_t most, size_t forced = 0) {
  if (forced >= 1 && forced <= most && (forced & (forced - 1)) == 0) return forced;
  size_t parts = 1;
  while (parts < most && segments * parts < want && (uint64_t)parts * 2 * 2 <= longest) parts *= 2;
  return parts;
}

// part g of a segment of len records: the records [g len / parts, (g + 1) len / parts) of the segment -- EMPTY when len < parts
// leaves nothing for it
struct RecPart {
  uint64_t s0, s1;
};
TC_HD RecPart rec_part(uint64_t len, size_t g, size_t parts) { return RecPart{g * len / parts, (g + 1) * len / parts}; }
// look-ups per column that the longest part of the segment makes: what every lane of a wave runs (the shorter parts mask)
TC_HD uint64_t rec_part_trips(uint64_t len, size_t parts) { return (len + parts - 1) / parts; }

// The PAIRED G1 sums of tc_verify_decryption_share_records_rlc_batch (k_msm.hip k_rec_*_g1_pair): every segment
// is summed twice with the same scalars -- half 0 over points_a, half 1 over points_b -- in one stage-T and one stage-L launch
// of 2 J logical segments.  The tables and digit codes of half 1 lie behind ALL of half 0's, at chunk offset `chunks` =
// first_chunk[J], so a half has the layout of a launch_rec_sum_g1 call and no two lanes share a byte.
constexpr size_t kRecPairPoint = 96;  // bytes of an encoded G1 result
// stage T: lane t < 2 chunks works on chunk t of half 0, or on chunk t - chunks of half 1
struct RecPairChunk {
  size_t half;
  uint64_t c;
};
TC_HD uint64_t rec_pair_tables_lanes(uint64_t chunks) { return 2 * chunks; }
TC_HD RecPairChunk rec_pair_chunk(uint64_t t, uint64_t chunks) { return t < chunks ? RecPairChunk{0, t} : RecPairChunk{1, t - chunks}; }
// the first table / code PLACE of a segment that starts at chunk `first` in its half
TC_HD uint64_t rec_pair_place(size_t half, uint64_t first, uint64_t chunks) { return (half * chunks + first) * kRecChunk; }
// stage L: `parts` lanes per sum (a power of two of at most 64), the two sums of a segment next to each other -- they have the
// same length, so the same trip count: lanes [2 j parts, (2 j + 1) parts) are half 0 of segment j, the next `parts` lanes half 1.
// A sum never spans two waves (parts divides 64 and its lanes start at a multiple of parts); with parts = 64 the halves of a
// segment are two whole waves.
struct RecPairLane {
  size_t j, half, g;
};
TC_HD size_t rec_pair_ladder_lanes(size_t J, size_t parts) { return 2 * J * parts; }
TC_HD RecPairLane rec_pair_lane(size_t lane, size_t parts) {
  const size_t q = lane / parts;
  return RecPairLane{q / 2, q % 2, lane % parts};
}
// where the leader lane of (segment j, half) writes: the operand array of the product check interleaves A_j and -B_j
TC_HD size_t rec_pair_out(size_t j, size_t half) { return (2 * j + half) * kRecPairPoint; }

}  // namespace tc
