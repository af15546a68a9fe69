// Host arithmetic of the combined entries of tc_api.hip -- "check a whole group with one pairing, re-check the failures one by
// one": how a batch is cut into groups, which jobs a failed group sends to the per-job checks, and the index maps that compact
// the N slots of every failed job.  Plain host C++, no HIP: tc_api.hip and tests/fallback/fallback_host.cpp (g++) share it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace tc {

// B jobs in groups of `group` consecutive jobs: G full groups, then `tail` < group jobs in a group of their own; NG groups in all
struct GroupCut {
  size_t group, G, tail, NG;
};
// the caller's `group` as the entries take it: 0 = the default of 64, at most 1024, at most B
inline GroupCut group_cut(size_t B, size_t group) {
  if (group == 0) group = 64;
  if (group > 1024) group = 1024;
  if (group > B) group = B;
  GroupCut c{group, 0, 0, 0};
  if (group) {
    c.G = B / group;
    c.tail = B % group;
    c.NG = c.G + (c.tail ? 1 : 0);
  }
  return c;
}

// appends to `out` every job of the groups g < cut.NG with bad_group[g] != 0, in order
inline void failed_jobs_of_groups(const uint8_t* bad_group, const GroupCut& cut, size_t B, std::vector<uint32_t>& out) {
  for (size_t g = 0; g < cut.NG; g++) {
    if (!bad_group[g]) continue;
    const size_t lo = g * cut.group, hi = (lo + cut.group < B) ? lo + cut.group : B;
    for (size_t j = lo; j < hi; j++) out.push_back((uint32_t)j);
  }
}

// The rows f * N + i of F failed jobs x N slots: the record (failed[f], i) of the call's B x N arrays, its job, its slot
struct SlotMaps {
  std::vector<uint32_t> record, job, slot;
};
inline SlotMaps slot_maps(const uint32_t* failed, size_t F, size_t N) {
  SlotMaps m;
  m.record.resize(F * N);
  m.job.resize(F * N);
  m.slot.resize(F * N);
  for (size_t f = 0; f < F; f++)
    for (size_t i = 0; i < N; i++) {
      m.record[f * N + i] = (uint32_t)(failed[f] * N + i);
      m.job[f * N + i] = failed[f];
      m.slot[f * N + i] = (uint32_t)i;
    }
  return m;
}

}  // namespace tc
