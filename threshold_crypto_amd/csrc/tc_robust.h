// Share selection of the robust combiners (tc_combine_signatures_robust_batch / tc_decrypt_robust_batch, k_robust.hip): which
// of a job's N slots go into the Lagrange combination.  A node holds up to N shares per message, slot i being node i's
// (abscissa i + 1); some are absent (`present`), some turned out invalid (`bad`).  The combination takes the FIRST `need` = t+1
// eligible slots in index order -- what the reference's BTreeMap iteration gives interpolate (src/lib.rs:608-615, 719-733).
// Plain host+device code (tests/robust/robust_host.cpp compiles it with g++).
#pragma once
#include "tc_common.h"

namespace tc {

// Scans the N mask bytes of one job.  Slot i is eligible when present_row[i] != 0 (a null present_row: every slot is present)
// and bad_row[i] == 0 (a null bad_row: nothing is bad).  Writes the first `need` eligible slot numbers to slot_out and the same
// numbers as abscissa indices to idx_out -- the u64 index i the combine kernels take and map to i + 1 themselves (tc_threshold.h
// lagrange: x = idx + 1), so nothing is added here.  Returns how many it wrote (<= need; the scan stops there) and writes
// nothing past them.  Rows may start at any byte offset (j * N need not be a multiple of 8): the bytes in front of the first
// 8-byte boundary and behind the last one are read one by one, the rest as 8-byte words -- N = 200 is 25 loads per mask -- when
// both rows sit at the same offset from a boundary, and bytewise otherwise.
TC_HD size_t select_first(const uint8_t* present_row, const uint8_t* bad_row, size_t N, size_t need, uint64_t* idx_out, uint32_t* slot_out) {
  size_t count = 0, i = 0;
  if (need == 0) return 0;
  const uint8_t* ref = present_row ? present_row : bad_row;
  if (!ref) {  // no mask at all: the first slots
    for (; i < N && count < need; i++, count++) {
      idx_out[count] = (uint64_t)i;
      slot_out[count] = (uint32_t)i;
    }
    return count;
  }
  const bool words = !present_row || !bad_row || ((((uintptr_t)present_row) ^ ((uintptr_t)bad_row)) & 7) == 0;
  size_t head = words ? (size_t)((8 - (((uintptr_t)ref) & 7)) & 7) : N;
  if (head > N) head = N;
  const size_t body_end = words ? head + ((N - head) & ~(size_t)7) : N;
  while (i < N) {
    if (i >= head && i < body_end) {
      // one aligned word of each mask: eight slots
      const uint64_t pw = present_row ? *reinterpret_cast<const uint64_t*>(present_row + i) : ~(uint64_t)0;
      const uint64_t bw = bad_row ? *reinterpret_cast<const uint64_t*>(bad_row + i) : 0;
      if (pw != 0) {
        for (int b = 0; b < 8; b++) {
          if (((pw >> (8 * b)) & 0xff) != 0 && ((bw >> (8 * b)) & 0xff) == 0) {
            idx_out[count] = (uint64_t)(i + b);
            slot_out[count] = (uint32_t)(i + b);
            if (++count == need) return count;
          }
        }
      }
      i += 8;
    } else {
      if ((!present_row || present_row[i] != 0) && (!bad_row || bad_row[i] == 0)) {
        idx_out[count] = (uint64_t)i;
        slot_out[count] = (uint32_t)i;
        if (++count == need) return count;
      }
      i++;
    }
  }
  return count;
}

// Where record i = j * need + k of the selected decode (k_decompress_selected, the wire forms of the robust combiners) finds
// its compressed share in the caller's jobs x N array of `cbytes`-byte encodings: the byte offset (j * N + slot[i]) * cbytes.
// A job without enough shares has no source -- its slots are 0xffffffff (k_select_shares) and are NOT read, no offset is
// formed from them: kNoSource, and the record is the identity.
constexpr size_t kNoSource = ~(size_t)0;
TC_HD size_t selected_source(size_t i, size_t N, size_t need, const uint32_t* slot, const uint8_t* enough, size_t cbytes) {
  const size_t j = i / need;
  if (!enough[j]) return kNoSource;
  return (j * N + (size_t)slot[i]) * cbytes;
}

// verdict of k_robust_finish for one job of a pass
enum RobustVerdict : uint8_t {
  kRobustNotEnough = 0,  // fewer than t+1 eligible shares
  kRobustGood = 1,       // combined, and the combination stands
  kRobustRetry = 2,      // enough shares, but the combination does not stand: share by share
};

}  // namespace tc
